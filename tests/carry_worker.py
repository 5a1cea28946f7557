"""one arm of the carried-launch test (tests/test_gpu_carry.py): the trainer's step (engine.TrainStep: two eager steps, then hipGraph
replays) for a few seeded steps in THIS process, whose environment carries the plan's switches; what a caller of the step receives
and how often the plan took each carried form go to <out>.

    python tests/carry_worker.py <out.pt> <profile> <B> <N> <steps> [<precision>]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out, profile, B, N, steps = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    precision = sys.argv[6] if len(sys.argv) > 6 else "bf16"
    import bench
    import parity_harness as H
    from pointcloudprocessing_amd import _lib
    from pointcloudprocessing_amd.engine import TrainStep
    from pointcloudprocessing_amd.optim import KerasAdam
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    dev = torch.device("cuda:0")
    spec, lw = H.PROFILES[profile]
    model = PointNet(bench.CCLS, bench.CSEG, 0.3, 42, precision=precision, device=dev)
    bench.pin_classification_head(model)
    H.apply_profile(model, spec)
    opt = KerasAdam(model.params_flat.data, 1e-4, 7000, 0.7)
    pc, y_cls, y_seg, se3 = bench.synth_batch(B, N, 20260001, dev)
    torch.manual_seed(20260002)          # TrainStep draws the seed of its dropout masks from torch's global generator
    ts = TrainStep(model, opt, B, N, lw, use_graph=True)
    ts.load(pc, y_cls, y_seg, se3)
    torch.cuda.set_stream(ts.stream)
    for _ in range(steps):
        ts.run()
    torch.cuda.synchronize()
    cls, seg, R = model._last
    torch.save({"params": model.params_flat.data.cpu(), "grads": model.grads_flat.cpu(), "loss_sums": model.scalars[:7].cpu(),
                "classification_output": cls.cpu(), "segmentation_output": seg.cpu(), "se3": R.cpu(), "mode": ts.mode,
                "plan_count": [int(_lib.lib().pn_model_plan_count(i)) for i in range(3)]}, out)


if __name__ == "__main__":
    main()
