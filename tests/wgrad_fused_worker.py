"""one arm of the fused weight-gradient test (tests/test_gpu_wgrad_fused.py): the trainer's step (engine.TrainStep: two eager steps, then
hipGraph replays) for a few seeded steps in THIS process, whose environment carries PN_WGRAD_FUSE; what a caller of the step receives,
how many data-gradient GEMMs were planned fused and how many steps were planned go to <out>.

    python tests/wgrad_fused_worker.py <out.pt> <profile> <B> <N> <steps>"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out, profile, B, N, steps = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    import bench
    import parity_harness as H
    from pointcloudprocessing_amd import _lib
    from pointcloudprocessing_amd.engine import TrainStep
    from pointcloudprocessing_amd.optim import KerasAdam
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet
    dev = torch.device("cuda:0")
    spec, lw = H.PROFILES[profile]
    model = PointNet(bench.CCLS, bench.CSEG, 0.3, 42, precision="bf16", device=dev)
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
    L = _lib.lib()
    torch.save({"params": model.params_flat.data.cpu(), "grads": model.grads_flat.cpu(), "loss_sums": model.scalars[:7].cpu(),
                "classification_output": cls.cpu(), "segmentation_output": seg.cpu(), "se3": R.cpu(), "mode": ts.mode,
                "fused_count": int(L.pn_model_wgrad_fused_count()),
                # the d(R_64) ride is planned once per planned backward pass (PN_DR64_RIDE, on by default): the number of planned steps
                "planned_steps": int(L.pn_model_plan_count(2))}, out)


if __name__ == "__main__":
    main()
