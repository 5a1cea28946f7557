"""GPU parity on the configurations BASELINE.json names, at their named sizes, and of the pieces every timed step runs
(Adam + ExponentialDecay, the orthogonality regularisers), against the CPU oracle.

PARITY UNPINNED against the reference itself (see tests/parity_harness.py): the checker is oracle/pointnet_oracle.py.

  C2  PointNet-cls  B=32, N=1024, bf16 MFMA operands, profile classification_pretrain  -- what bench.py times
  C3  PointNet-seg  B=32, N=2048, profile final (segmentation head trained)             -- bf16x3 and bf16
  C4  PointNet-cls  per-rank shape of the 8-GPU run: B=8, N=4096                        -- bf16x3 and bf16
  C1  the trainer entry point at its named size (N=1024, batch 4) is in tests/test_gpu_train.py

How it is checked (tests/parity_harness.py and tests/teacher_forced.py have the reasoning):
  * teacher-forced, layer by layer: every layer of the step recomputed in fp64 from the GPU's own stored input of that layer, forward
    and backward, fixed tolerances of a few units in the last place of the storage type (2^-8 / 2^-7 of the tensor maximum for
    bf16-stored tensors, 1e-4 .. 2e-3 for fp32 ones).  Run on the SURVEY 8d clouds bench.py times AND on shape-diverse clouds;
  * end to end against oracle B (fp64, the mode's roundings emulated, the GPU's discrete decisions imposed): a quantity passes within
    max(absolute tolerance, 4 x floor), floor = |oracle B run in fp32 - oracle B| = what any two correct implementations of the mode
    differ by on these inputs.  Absolute tolerances: bf16x3 gradients 5e-3 of each tensor's max and training-mode outputs 3e-4; bf16
    gradients 2e-2, outputs 5e-3.  Run on the shape-diverse clouds with the T-Net tails damped (R close to the identity `b`, as in a
    regularised trained model): there the RMS limit on a probability stays below 1e-2 in every configuration;
  * inference (training=False) at the BASELINE sizes against the fp64 oracle with north_star's numbers: probabilities within 1e-3,
    class index bit-exact, part index bit-exact wherever the oracle's own top-2 margin exceeds the tolerance.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pointnet_oracle as O   # noqa: E402  (checker only)
from parity_harness import BF16, CCLS, CSEG, X3, build_model, check_training_step, make_inputs, report   # noqa: E402


@pytest.mark.parametrize("name,B,N,profile,precision,tol", [
    ("C2", 32, 1024, "classification_pretrain", "bf16", BF16),
    ("C2-x3", 32, 1024, "classification_pretrain", "bf16x3", X3),
    ("C3", 32, 2048, "final", "bf16x3", X3),
    ("C3-bf16", 32, 2048, "final", "bf16", BF16),
    ("C4-rank", 8, 4096, "classification_pretrain", "bf16x3", X3),
    ("C4-rank-bf16", 8, 4096, "classification_pretrain", "bf16", BF16),
])
def test_training_step_at_baseline_config(dev, name, B, N, profile, precision, tol):
    # (1) the clouds bench.py times: every layer teacher-forced (no end-to-end comparison: on near-identical clouds the batch statistics
    #     of the per-cloud dense layers amplify the mode's rounding to 0.2 in probability -- nothing to assert there)
    check_training_step(dev, B, N, profile, precision=precision, seed_params=21, seed_inputs=20260001, inputs="survey", end_to_end=False,
                        tag=f"{name}/survey[{profile},{precision},B={B},N={N}]", **tol)
    # (2) shape-diverse clouds, T-Net tails damped: teacher-forced AND end to end
    worst, _ = check_training_step(dev, B, N, profile, precision=precision, seed_params=21, seed_inputs=20260002, inputs="shapes", damp_tnet=0.1,
                                   tag=f"{name}[{profile},{precision},B={B},N={N}]", **tol)
    report(f"{name}: worst relative gradient error {worst:.3e} (tolerance {tol['tol_grad']:.0e})")


@pytest.mark.parametrize("name,B,N,vanilla", [("C2", 32, 1024, False), ("C3", 32, 2048, False), ("C4-rank", 8, 4096, False),
                                              ("C5-sampled", 1, 8192, True)])
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_inference_at_baseline_size(dev, name, B, N, vanilla, precision):
    """training=False at the BASELINE shapes against the fp64 oracle (PointNet.py:197-292 with moving statistics), north_star's
    acceptance: probabilities and R within 1e-3, arg-max class bit-exact, per-point part index bit-exact wherever the oracle's own
    top-2 margin exceeds twice the error bound (closer than that the two maxima are a tie at the stated tolerance).  C5-sampled: one
    cloud of M = 8192 points drawn from the kc-46 hull (what voxel grid + FPS hand to the network), vanilla as tools/bench_scan.py.
    Weights: seeded, BatchNormalization parameters and moving statistics perturbed (randomize_bn) so every term is exercised."""
    params = O.init_params(CCLS, CSEG, seed=23, vanilla=vanilla, randomize_bn=True)
    if name == "C5-sampled":
        import numpy as np, os
        pts = []
        for ln in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kc-46.txt")):
            pts.append([float(v) for v in ln[ln.index("(") + 1: ln.index(")")].split(",")])
        hull = torch.tensor(pts, dtype=torch.float32)
        g = torch.Generator().manual_seed(5)
        pc = (hull[torch.randint(0, hull.shape[0], (N,), generator=g)] + 0.15 * torch.randn(N, 3, generator=g)).unsqueeze(0).contiguous()
    else:
        pc, *_ = make_inputs(B, N, 20260001, "survey")
    ref = O.forward({k: v.double() for k, v in params.items()}, pc.double(), training=False, vanilla=vanilla)
    m = build_model(dev, params, vanilla, precision=precision)
    cls, seg, R = m(pc.to(dev), training=False)
    ci, si, _ = m.predict(pc.to(dev))
    cls, seg, R = cls.cpu().double(), seg.cpu().double(), R.cpu().double()
    e = [float((cls - ref[0]).abs().max()), float((seg - ref[1]).abs().max()), float((R - ref[2]).abs().max())]
    rms = [float((cls - ref[0]).pow(2).mean().sqrt()), float((seg - ref[1]).pow(2).mean().sqrt())]
    report(f"inference {name} {precision} B={B} N={N}: max abs err cls {e[0]:.3e} seg {e[1]:.3e} R {e[2]:.3e}; RMS cls {rms[0]:.3e} seg {rms[1]:.3e}")
    # north_star's 1e-3 holds in BOTH modes.  Measured (round 3, gpurun_out/model_report.txt): bf16x3 6e-7 / 1.6e-6 / 7e-6 (class / part /
    # R); bf16 (bf16 MFMA operands AND bf16 layer-boundary tensors) 1.0e-4 / 8.4e-4 / 9.0e-4, RMS of the part probabilities 1.3e-4 --
    # the fp64 oracle itself moves by about as much when its operands are rounded the same way (oracle A vs B on the CPU: 1.6e-4 / 1.3e-3
    # / 1.0e-3).  R is a 3x3 matrix with entries of order 1, not a probability: its bf16 tolerance is 1.5e-3.
    t_cls, t_seg, t_R, t_rms = (1e-3, 1e-3, 1.5e-3, 3e-4) if precision == "bf16" else (2e-5, 2e-5, 2e-5, 2e-6)
    assert e[0] < t_cls and e[1] < t_seg and e[2] < t_R and rms[1] < t_rms, (name, precision, e, rms)
    assert torch.equal(cls.argmax(-1), ref[0].argmax(-1)) and torch.equal(ci.cpu().long(), ref[0].argmax(-1))
    top2 = ref[1].topk(2, dim=-1).values
    safe = (top2[..., 0] - top2[..., 1]) > 2 * max(e[1], 1e-6)
    assert float(safe.double().mean()) > 0.97, float(safe.double().mean())
    assert torch.equal(seg.argmax(-1)[safe], ref[1].argmax(-1)[safe]) and torch.equal(si.cpu().long()[safe], ref[1].argmax(-1)[safe])


def test_both_regularisers_on(dev):
    """regularize_input_transform / regularize_feature_transform (PointNet.py:92-93, 447-451): 1e-3 * l2_loss(I - R R^T) summed over the
    batch enters the loss through add_loss; scalars[5], scalars[6] and every T-Net gradient against the oracle.  The T-Net tail `b` is
    perturbed away from the identity (init_params randomize_bn) so that I - R R^T is not ~0."""
    worst, m = check_training_step(dev, 16, 136, "all", precision="bf16x3", reg=True, seed_params=31, seed_inputs=32)
    sc = m.scalars.cpu()
    assert float(sc[5]) > 0 and float(sc[6]) > 0
    # the regularisers alone must reach the T-Nets: zero loss weights, heads frozen -> only add_loss terms drive the gradients
    worst2, m2 = check_training_step(dev, 16, 136, "reg_only", precision="bf16x3", reg=True, seed_params=31, seed_inputs=32)
    assert float(m2.named_grads()["feature_transform.w"].abs().max()) > 0


def test_adam_kernel_matches_keras_adam(dev):
    """pn_adam_step (the one launch every timed step ends with: device-side ExponentialDecay schedule, last-ticket iteration advance,
    grad_scale) against oracle.keras_adam_step + exponential_decay_lr (pointnet_train.py:310-319) over 5 steps, one of them with
    grad_scale = 0.5 (the 1/world of a two-rank sum), then a restore of (m, v, iterations) into a fresh optimizer and 3 more steps."""
    from pointcloudprocessing_amd.optim import KerasAdam
    n = 4_210_476 + 13                                        # the model's parameter count, not a multiple of the block size
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g) * 0.1
    lr0, ds, dr = 1e-3, 7.0, 0.7                             # a short decay period so that the schedule moves visibly within 8 steps
    p_ref, m_ref, v_ref = p0.double().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p_gpu = p0.to(dev).clone()
    opt = KerasAdam(p_gpu, lr0, ds, dr)
    scales = [1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 0.25, 1.0]
    for step, gs in enumerate(scales):
        grad = torch.randn(n, generator=g) * (10.0 ** (step % 3 - 2))      # magnitudes 1e-2 .. 1
        if step == 5:                                          # checkpoint restore into a new optimizer object
            state = {k: v.clone() for k, v in opt.state_dict().items()}
            opt = KerasAdam(p_gpu, lr0, ds, dr)
            assert int(opt.iterations) == 0
            opt.load_state_dict(state)
            assert int(opt.iterations) == 5
        lr = O.exponential_decay_lr(lr0, step, ds, dr)
        assert abs(opt.learning_rate - lr) < 1e-6 * lr, (step, opt.learning_rate, lr)
        opt.step(grad.to(dev), gs)
        O.keras_adam_step(p_ref, grad.double() * gs, m_ref, v_ref, step, lr)
        torch.cuda.synchronize()
        assert int(opt.iterations) == step + 1
        ep = float((p_gpu.cpu().double() - p_ref).abs().max())
        em = float((opt.m.cpu().double() - m_ref).abs().max() / m_ref.abs().max())
        ev = float((opt.v.cpu().double() - v_ref).abs().max() / v_ref.abs().max())
        report(f"adam step {step}: max abs param err {ep:.3e}, rel m err {em:.3e}, rel v err {ev:.3e}, lr {lr:.6e}")
        # fp32 state against fp64: a step moves a parameter by at most ~lr, and its rounding error is a few ulp of the parameter
        assert ep < 5e-7 and em < 1e-5 and ev < 1e-5, (step, ep, em, ev)
    moved = float((p_gpu.cpu().double() - p0.double()).abs().max())
    assert moved > 3 * lr0                                     # the comparison above is not vacuous
    assert math.isclose(opt.learning_rate, O.exponential_decay_lr(lr0, len(scales), ds, dr), rel_tol=1e-6)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 2 * 256 * 1024 * 4 + 7])
def test_adam_kernel_on_small_and_misaligned_ranges(dev, n):
    """pn_adam_step over a range [lo, hi) of the flat buffers (KerasAdam.step(lo=..., hi=...)) whose four arrays start 0 .. 3 floats
    into 16-byte-aligned buffers: the launcher takes the 16-byte path only when all four pointers are aligned (vec = 1) and the scalar
    path otherwise (vec = 0); n < 4 has no quad, n % 4 a scalar tail, n <= 1024 a grid of one block, 1025 of two, and the largest n one
    quad more than two full grid strides (one thread goes round again with a single quad in flight).  Two steps, the second with
    grad_scale = 0.5.  Every placement against oracle.keras_adam_step in fp64 (the limits of test_adam_kernel_matches_keras_adam);
    every misaligned placement equals the aligned one BIT FOR BIT (the per-element arithmetic is the same lambda); the floats before lo
    and after hi keep their bits; iterations advances by one per step and the ticket word is back at 0."""
    from pointcloudprocessing_amd.optim import KerasAdam
    g = torch.Generator().manual_seed(1000 + n % 997)
    lr0, ds, dr = 1e-3, 7.0, 0.7
    lo, pad = 4, 8                                             # floats in front of / behind the range
    p0 = torch.randn(n, generator=g) * 0.1
    g_prev = torch.randn(n, generator=g) * 0.1                 # moments of an optimizer in flight (not the zeros of a fresh one), consistent
    m0, v0 = 0.1 * g_prev, 1e-3 * g_prev * g_prev              # with one another: m / sqrt(v) stays bounded, a step moves a parameter by ~lr
    grads = [torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g)]
    scales = [1.0, 0.5]
    p_ref, m_ref, v_ref = p0.double().clone(), m0.double().clone(), v0.double().clone()
    refs = []
    for step, (gr, gs) in enumerate(zip(grads, scales)):
        O.keras_adam_step(p_ref, gr.double() * gs, m_ref, v_ref, step, O.exponential_decay_lr(lr0, step, ds, dr))
        refs.append((p_ref.clone(), m_ref.clone(), v_ref.clone()))

    def placed(values, off, fill):
        """an aligned buffer holding `values` from float off + lo on; returns (the view the optimizer gets, the whole buffer's start)"""
        buf = torch.full((4 + lo + n + pad,), fill, dtype=torch.float32)
        buf[off + lo: off + lo + n] = values
        buf = buf.to(dev)
        assert buf.data_ptr() % 16 == 0
        return buf[off: off + lo + n + pad - 4], buf

    first = None
    # (p, g, m, v) offsets in floats: all aligned (vec = 1), then each array alone off by 1 .. 3, all off by the same, all different
    for offs in [(0, 0, 0, 0), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (2, 2, 2, 2), (1, 2, 3, 0), (3, 1, 0, 2)]:
        pv, pbuf = placed(p0, offs[0], 7.0)
        mv, mbuf = placed(m0, offs[2], 5.0)
        vv, vbuf = placed(v0, offs[3], 3.0)
        opt = KerasAdam(pv, lr0, ds, dr)
        opt.m, opt.v = mv, vv
        aligned = all((t.data_ptr() + 4 * lo) % 16 == 0 for t in (pv, mv, vv))
        for step, (gr, gs) in enumerate(zip(grads, scales)):
            gv, gbuf = placed(gr, offs[1], 9.0)
            g_before = gbuf.clone()
            assert (aligned and (gv.data_ptr() + 4 * lo) % 16 == 0) == (offs == (0, 0, 0, 0))
            opt.step(gv, gs, lo=lo, hi=lo + n)
            torch.cuda.synchronize()
            assert int(opt.iterations) == step + 1, (n, offs, step, int(opt.iterations))
            assert int(opt._alpha.view(torch.int32)[2]) == 0, (n, offs, step)
            assert torch.equal(gbuf, g_before), (n, offs, "the gradient was written")
            got = [t[lo: lo + n].cpu() for t in (pv, mv, vv)]
            pr, mr, vr = refs[step]
            ep = float((got[0].double() - pr).abs().max())
            em = float((got[1].double() - mr).abs().max() / mr.abs().max())
            ev = float((got[2].double() - vr).abs().max() / vr.abs().max())
            if step == 1:
                report(f"adam range n={n} offsets {offs}: max abs param err {ep:.3e}, rel m err {em:.3e}, rel v err {ev:.3e}")
            assert ep < 5e-7 and em < 1e-5 and ev < 1e-5, (n, offs, step, ep, em, ev)
            for (view, buf), off, fill in (((pv, pbuf), offs[0], 7.0), ((mv, mbuf), offs[2], 5.0), ((vv, vbuf), offs[3], 3.0)):
                whole = buf.cpu()
                assert bool((whole[: off + lo] == fill).all()) and bool((whole[off + lo + n:] == fill).all()), (n, offs, step, "outside [lo, hi)")
        assert float((got[0] - p0).abs().max()) > 0
        if first is None:
            first = got
        else:
            assert all(torch.equal(a, b) for a, b in zip(got, first)), (n, offs, "differs from the aligned placement")


def test_nan_and_inf_clouds_do_not_fault(dev):
    """regression (round 1, gpurun call 20): a cloud holding NaN made every arg-max comparison false, the index sentinel 0x7fffffff
    reached the scatter of the max-pool backward and the GPU faulted.  A NaN cloud and an Inf cloud through fused_loss_step: no fault,
    every arg-max index inside the cloud, the loss sums flagged non-finite, and the healthy step afterwards is unaffected."""
    B, N = 4, 300
    params = O.init_params(CCLS, CSEG, seed=41, randomize_bn=True)
    pc, y_cls, y_seg, se3, keep = make_inputs(B, N, 42)
    kp = (keep["dropout_1"].to(torch.uint8).to(dev), keep["dropout_2"].to(torch.uint8).to(dev))
    args = (y_cls.to(torch.int32).to(dev), y_seg.to(torch.int32).to(dev), se3.to(dev), (1.0, 1.0, 1.0))
    m = build_model(dev, params, precision="bf16")
    m.fused_loss_step(pc.to(dev), *args, keep=kp)
    torch.cuda.synchronize()
    healthy = m.grads_flat.clone()
    assert bool(torch.isfinite(healthy).all())
    for poison in (float("nan"), float("inf"), -float("inf")):
        bad = pc.clone()
        bad[1, 17, 2] = poison
        bad[3, :, :] = poison                                   # a whole cloud
        m.set_weights(params)                                   # moving statistics back to finite values
        m.fused_loss_step(bad.to(dev), *args, keep=kp)
        torch.cuda.synchronize()
        for wn in ("iT.m3", "fT.m3", "mm23"):
            arg = m.workspace_tensor(wn + ".arg", B, N, True, torch.int32)
            assert int(arg.min()) >= 0 and int(arg.max()) < N, (poison, wn, int(arg.min()), int(arg.max()))
        sc = m.scalars.cpu()
        assert not bool(torch.isfinite(sc[[0, 2]]).all()), (poison, sc.tolist())
    m.set_weights(params)
    m.fused_loss_step(pc.to(dev), *args, keep=kp)
    torch.cuda.synchronize()
    assert torch.equal(m.grads_flat, healthy)


def test_debugging_flag_checks_numerics(dev):
    """`debugging: true` (pointnet_train.py:112) makes the reference wrap every layer output in tf.debugging.check_numerics
    (PointNet.py:199-288): the first layer whose output holds a NaN / Inf raises, named.  Off: no check, no error."""
    from pointcloudprocessing_amd._lib import PointNetHipError
    B, N = 2, 200
    params = O.init_params(CCLS, CSEG, seed=43, randomize_bn=True)
    pc, *_ = make_inputs(B, N, 44)
    m = build_model(dev, params, precision="bf16", debugging=True)
    m(pc.to(dev), training=False)                               # healthy input passes
    bad = pc.clone()
    bad[0, 5, 1] = float("nan")
    with pytest.raises(PointNetHipError, match="Input point cloud contains nan values"):
        m(bad.to(dev), training=False)
    # a poisoned weight deeper in the network is blamed on that layer, not on an earlier one
    p2 = {k: v.clone() for k, v in params.items()}
    p2["mlp_2_2.kernel"][3, 7] = float("inf")
    m2 = build_model(dev, p2, precision="bf16", debugging=True)
    with pytest.raises(PointNetHipError, match="mlp_2_2 produced nan values"):
        m2(pc.to(dev), training=False)
    m3 = build_model(dev, p2, precision="bf16", debugging=False)
    m3(pc.to(dev), training=False)                              # no check without the flag (the reference behaves the same)
