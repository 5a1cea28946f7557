"""one arm of the plan-arm tests (tests/test_gpu_plan_arms.py): every case of a list in THIS process, whose environment carries the arm's
switches (they are read once per process; this file reads none).  One record per case goes to <out.pt>.

    python tests/plan_arm_worker.py <out.pt> <mode> <cases.json>

mode 'train':     case [B, N, profile, vanilla, precision]: parity_harness.check_training_step exactly as tests/test_gpu_large_batch.py
                  calls it (every layer teacher-forced in fp64 + the whole step against the oracle, the project's tolerances); with a
                  sixth element "ragged": on the clouds of tests/test_gpu_long_clouds.py, teacher-forced only;
mode 'seghead':   case [B, N, vanilla]: the fused frozen segmentation head against the layer-by-layer plan (tests/test_gpu_model.py);
mode 'infer':     case [B, N, vanilla]: bf16 inference on seeded weights over a poisoned workspace;
mode 'dense_ops': no cases: the dense layers' op-level checks of tests/test_gpu_ops.py at their own parametrisations.

An AssertionError of a check is recorded with its text under the case and the worker exits 1 AFTER writing the file; anything else
propagates."""
import json
import os
import sys
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _counts():
    from pointcloudprocessing_amd import _lib
    L = _lib.lib()
    return [int(L.pn_model_plan_count(i)) for i in range(3)] + [int(L.pn_model_wgrad_fused_count())]


def train_case(dev, case):
    import parity_harness as H
    B, N, profile, vanilla, precision = case[:5]
    # a sixth element "ragged": the clouds of tests/test_gpu_long_clouds.py (the farthest points in the ragged last tile), teacher-forced
    # only -- two or three clouds leave the whole-step comparison ill-conditioned
    ragged = len(case) > 5 and case[5] == "ragged"
    assert len(case) == 5 or ragged, case
    tol = {"bf16x3": H.X3, "bf16": H.BF16}
    before = _counts()
    _, m = H.check_training_step(dev, B, N, profile, vanilla=vanilla, precision=precision, seed_params=21, seed_inputs=20260003,
                                 inputs="shapes", damp_tnet=0.1, tag=f"plan-arm[{profile},vanilla={vanilla},{precision},B={B},N={N}]",
                                 end_to_end=not ragged, pc_hook=H.farthest_point_last if ragged else None, **tol[precision])
    if ragged:
        for wn in ("mm23",) if vanilla else ("mm23", "iT.m3", "fT.m3"):
            hits = H.ragged_tile_hits(m.workspace_tensor(wn + ".arg", B, N, True, torch.int32).view(B, 1024).cpu(), N)
            assert int(hits.min()) >= 64, (wn, hits.tolist())
    after = _counts()
    # the witness: check_training_step poisoned the workspace with 0xFF before the step -- did anything write the Pm slabs?
    pm = m.workspace_tensor("pm_slabs", B, N, True, torch.uint8)
    witness = "poison" if bool((pm == 255).all()) else ("finite" if bool(torch.isfinite(pm.view(torch.float32)).all()) else "mixed")
    cls, seg, R = m._last
    return {"grads": m.grads_flat.cpu(), "classification_output": cls.cpu(), "segmentation_output": seg.cpu(), "se3": R.cpu(),
            "loss_sums": m.scalars[:7].cpu(), "plan_count": [a - b for a, b in zip(after[:3], before[:3])],
            "wgrad_fused_count": after[3] - before[3], "pm_slabs": witness}


def seghead_case(dev, case):
    from test_gpu_model import fused_head_against_layer_by_layer
    B, N, vanilla = case
    (inf, tr, grads, scalars), _, _ = fused_head_against_layer_by_layer(dev, vanilla, B, N)
    return {"inference": [t.cpu() for t in inf], "training": [t.cpu() for t in tr], "grads": grads.cpu(), "loss_sums": scalars.cpu()}


def infer_case(dev, case):
    import parity_harness as H
    from oracle import pointnet_oracle as O
    from test_gpu_model import _ws_entries
    B, N, vanilla = case
    params = O.init_params(H.CCLS, H.CSEG, seed=21, vanilla=vanilla, randomize_bn=True)
    pc = H.make_inputs(B, N, 20260006, "shapes")[0].to(dev)
    m = H.build_model(dev, params, vanilla, precision="bf16")
    ws = m._workspace(B, N, False)
    ws.fill_(255)
    outs = [t.clone() for t in m(pc, training=False)]
    torch.cuda.synchronize()
    written = {name: bool((ws[off: off + nb] != 255).any()) for name, off, nb in _ws_entries(m, B, N, False)}
    return {"outputs": [t.cpu() for t in outs], "written": written}


def dense_ops_cases():
    import test_gpu_ops as T

    def params_of(fn):
        return [mk for mk in fn.pytestmark if mk.name == "parametrize"][0].args[1]
    out = []
    for p in params_of(T.test_dense_layer_matches_fp64_reference):
        out.append((("dense_layer",) + tuple(p), lambda dev, p=p: T.test_dense_layer_matches_fp64_reference(dev, *p)))
    for p in T.DENSE_BWD_CASES:
        out.append((("dense_bwd",) + tuple(p), lambda dev, p=p: T.check_dense_bwd(dev, *p)))
    for p in params_of(T.test_dense_backward_chain_step_equals_the_two_launch_form):
        out.append((("dense_bwd_step",) + tuple(p), lambda dev, p=p: T.test_dense_backward_chain_step_equals_the_two_launch_form(dev, *p)))
    return out


def main():
    out, mode = sys.argv[1], sys.argv[2]
    with open(sys.argv[3]) as f:
        cases = json.load(f)
    dev = torch.device("cuda:0")
    if mode == "dense_ops":
        jobs = [(list(k), lambda dev, fn=fn: fn(dev) or {}) for k, fn in dense_ops_cases()]
    else:
        run = {"train": train_case, "seghead": seghead_case, "infer": infer_case}[mode]
        jobs = [(c, lambda dev, c=c: run(dev, c)) for c in cases]
    records, failed = [], False
    for case, job in jobs:
        rec = {"case": list(case), "error": None}
        try:
            rec.update(job(dev))
        except AssertionError:
            rec["error"] = traceback.format_exc()[-3000:]
            failed = True
        records.append(rec)
    torch.save(records, out)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
