"""`PointNet(..., training=False)` and `predict` on the HIP path against the fp64 oracle at the shapes of tests/inference_cases.py: clouds
shorter than one 64-row slot of chain_max_kernel (pn_panel.hip), a one-row slot behind a whole one, either side of the 128-row tiles,
more than 32 and more than 128 clouds in the moving-statistics dense layers, one long ragged cloud -- what a cluster-labelling call
hands the network and no BASELINE configuration has.  tests/test_cpu_inference_cases.py shows without a GPU that the oracle's arg-max
indices are clear of ties at these cases, so the index comparisons below mean something.

PARITY UNPINNED against the reference itself (no TF here): the checker is oracle/pointnet_oracle.py.  The kernels these shapes isolate
are compared bit for bit with the launches they replace in tests/test_gpu_ops.py (the chain kernel) and tests/test_gpu_model.py /
tests/test_gpu_plan_arms.py (the fused segmentation head) at the same shapes: a wrong number here that those two pass is in the dense
layers, the normalisation or the softmax.
"""
import pytest
import torch

import inference_cases as IC
from parity_harness import build_model, report

pytestmark = pytest.mark.gpu


def _errors(outs, ref):
    return [float((o.cpu().double() - r).abs().max()) for o, r in zip(outs, ref)]


def _run_poisoned(m, fn, pc):
    """every byte of the inference workspace 0xFF (NaN as fp32 and as bf16, -1 as an index) before the call, as plan_arm_worker.infer_case
    does: a padded row or a stale entry that is read shows up as NaN in the outputs"""
    B, N, _ = pc.shape
    m._workspace(B, N, False).fill_(255)
    out = fn(pc)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("vanilla", [False, True])
@pytest.mark.parametrize("B,N", IC.SHAPES, ids=IC.IDS)
def test_inference_matches_the_fp64_oracle_at_short_ragged_and_large_batches(dev, B, N, vanilla, precision):
    """Max abs error of class, part and R against the fp64 oracle under the mode's bound (inference_cases.bounds: 'bf16x3' 2e-4 for all
    three; 'bf16' max(1e-3 | 1e-3 | 1.5e-3, 4 x the case's bf16 floor)); finite outputs and probability rows that sum to 1 over a
    poisoned workspace; the class index the oracle's, the part index the oracle's at every point whose oracle margin exceeds twice the
    bound (at least 97 % of them); `predict` the arg-max of the device's own probabilities; no weight or moving statistic touched; for
    (5, 31) and (40, 72) every cloud run alone at B = 1 equals its rows of the batch run within the same bound (moving statistics make
    the clouds independent).

    Measured on the MI355X, largest over the nine shapes and both model kinds (class / part / R), all three at (130, 40) with T-Nets:
        bf16x3   6.1e-7 / 1.4e-6 / 1.0e-5      (bound 2e-4)
        bf16     1.1e-4 / 6.9e-4 / 1.2e-3      (bounds there 1.0e-3 / 1.6e-3 / 3.6e-3; the case's floors 8.3e-5 / 4.1e-4 / 9.0e-4)
    Every 'bf16' error is within 2.3 x the bf16 floor of its own case (the widest ratio: the part probabilities of the one-point cloud,
    4.0e-4 against a floor of 1.7e-4).  Every cloud alone at B = 1 equalled its rows of the batch run bit for bit in both modes
    (reported, not asserted).
    With the first padded row of a ragged slot let into chain_max_kernel's pool (a scratch build) every 'bf16' case but (2, 64) fails
    here with class / part errors of 1.5e-3 .. 5.3e-3, and the x64 fronts of the chain test fail at every ragged shape.
    """
    case = (B, N, vanilla)
    exp = IC.expected(case)
    ref = exp["fp64"]
    b = IC.bounds(case, precision)
    tag = f"inference-shapes {precision} vanilla={vanilla} B={B} N={N}"
    m = build_model(dev, IC.weights(vanilla), vanilla, precision=precision)
    pc = IC.clouds(B, N).to(dev)
    before = m.params_flat.detach().clone()
    outs = [t.clone() for t in _run_poisoned(m, lambda x: m(x, training=False), pc)]
    ci, si, R2 = _run_poisoned(m, m.predict, pc)
    cls, seg, R = outs
    # finiteness
    assert all(bool(torch.isfinite(t).all()) for t in outs), [int((~torch.isfinite(t)).sum()) for t in outs]
    assert float((cls.sum(-1) - 1).abs().max()) < 1e-4 and float((seg.sum(-1) - 1).abs().max()) < 1e-4
    # error against the fp64 oracle
    e = _errors(outs, ref)
    report(f"{tag}: max abs err cls {e[0]:.3e} seg {e[1]:.3e} R {e[2]:.3e}; bounds {b[0]:.3e} {b[1]:.3e} {b[2]:.3e}; bf16 floor "
           f"{exp['floor_bf16'][0]:.3e} {exp['floor_bf16'][1]:.3e} {exp['floor_bf16'][2]:.3e}")
    print(f"{tag}: err {e} bounds {b}")
    assert e[0] < b[0] and e[1] < b[1] and e[2] < b[2], (tag, e, b)
    # indices
    cls_c, seg_c = cls.cpu(), seg.cpu()
    assert torch.equal(cls_c.argmax(-1), ref[0].argmax(-1))
    safe = IC.top2_margin(ref[1]) > 2 * b[1]
    assert float(safe.double().mean()) >= IC.SAFE_SHARE, float(safe.double().mean())
    assert torch.equal(seg_c.argmax(-1)[safe], ref[1].argmax(-1)[safe])
    # predict: the arg-max of the device's own probabilities, wherever its top two differ (a tie goes to the first, which torch.argmax
    # does not promise)
    assert ci.dtype == torch.int32 and si.dtype == torch.int32 and tuple(ci.shape) == (B,) and tuple(si.shape) == (B, N)
    assert torch.equal(R2, R)
    clear_c, clear_s = IC.top2_margin(cls_c) > 0, IC.top2_margin(seg_c) > 0
    assert torch.equal(ci.cpu().long()[clear_c], cls_c.argmax(-1)[clear_c]) and torch.equal(si.cpu().long()[clear_s], seg_c.argmax(-1)[clear_s])
    assert int(si.min()) >= 0 and int(si.max()) < 12 and int(ci.min()) >= 0 and int(ci.max()) < 23
    # state: moving statistics and every other weight byte for byte
    assert torch.equal(m.params_flat.detach().view(torch.int32), before.view(torch.int32))
    # per-cloud independence
    if (B, N) in IC.INDEPENDENT:
        worst, exact = [0.0, 0.0, 0.0], True
        for i in range(B):
            alone = _run_poisoned(m, lambda x: m(x, training=False), pc[i:i + 1].contiguous())
            for q, (a_, full) in enumerate(zip(alone, outs)):
                worst[q] = max(worst[q], float((a_[0].double() - full[i].double()).abs().max()))
                exact = exact and torch.equal(a_[0], full[i])
            assert all(bool(torch.isfinite(t).all()) for t in alone), i
        report(f"{tag}: every cloud alone at B=1 against its rows of the batch run: max abs diff cls {worst[0]:.3e} seg {worst[1]:.3e} "
               f"R {worst[2]:.3e}; {'bit for bit' if exact else 'NOT bit for bit'}")
        print(f"{tag}: alone vs batch {worst} exact={exact}")
        assert worst[0] < b[0] and worst[1] < b[1] and worst[2] < b[2], (tag, worst, b)
