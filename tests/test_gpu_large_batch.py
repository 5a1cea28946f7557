"""The training step where more than 32 rows reach the per-cloud dense layers, with a batch of one, and on clouds shorter than a tile.

The plan has two backward passes for the per-cloud dense layers (classification head, both T-Net tails), chosen by the number of rows
Bd = B * sync_world that reach them (pn_model.hip: bwd_dense, chain_ok, bwd_tnet, the has_cls block of backward_body):
  Bd <= 32  one launch per layer of a backward chain + one batched weight-gradient launch;
  Bd  > 32  per layer dense_bwd_pre (dropout / ReLU / BatchNormalization backward over all rows), dense_wgrad on the auxiliary stream
            (fp32 fma chains over 32-row chunks; for the T-Net's X @ w + b also the column sums of dR) and a plain transposed product.
Every other parity test of a training step has B <= 32.  Here the second form is judged
  * at op level through pn_dense_bwd (which runs the same two launches for R > 32): exactly on small integers below, and against fp64
    autograd in tests/test_gpu_ops.py::test_dense_bwd_matches_autograd (R = 33, 40, 64, 257);
  * in whole steps at B = 33, 40, 64 by tests/parity_harness.py: every layer teacher-forced from the GPU's own stored inputs (the lines
    "d(mlp_cls_2 output)", "d(mlp_cls_1 output)", "d(global feature) from the classification head", "<tnet> d(dense2 output)",
    "<tnet> d(dense1 output)" and the dense layers' dz / dgamma / dbeta / dbias / dw lines are the ones this branch writes), and end to end
    against the oracle with the measured floor;
  * across the step layouts (hipGraph x auxiliary stream x split optimizer): the weight gradients of this form run on the auxiliary
    stream, so a missing join would be a race only here.
Next to it: B = 1 (dense-layer batch statistics over one row: variance 0, the gradient through the BatchNormalization identically 0) and
N < 128 / < 64 / < 32 (one partial statistics tile / a partial panel / a partial arg-max block) in the plan with its workspace layout,
which only op-level tests reached.  These are teacher-forced only: the whole-step comparison is ill-conditioned at such batches.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from parity_harness import BF16, X3, check_training_step, report   # noqa: E402
from test_gpu_ops import _ops, check_dense_bwd, ints            # noqa: E402

TOL = {"bf16x3": X3, "bf16": BF16}


# ---------------------------------------------------------------------------------------------------------------------
# op level: pn_dense_bwd with more than 32 rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bn_mode", [0, 2])
@pytest.mark.parametrize("R,K,C_", [(33, 130, 23), (40, 9, 70), (64, 1024, 512), (257, 130, 70), (17, 64, 96)])
def test_dense_bwd_exact_on_integers(dev, R, K, C_, bn_mode):
    """integer x and da, a 0/1 keep mask with rate 0.5 (keep_scale 2), no BatchNormalization (bn_mode 0) or moving statistics with
    invstd = 1, mean = 0 and gamma a power of two (bn_mode 2): every product and every partial sum is an integer multiple of 1/4 below
    2^24, exact in fp32 whatever the order.  dz, dbias and dw must EQUAL the integer result: a swapped index, a 32-row chunk counted
    twice or a dropped last row is a hard mismatch.  (17 rows: the fused one-launch form, exact too with its split-bf16 operands.)"""
    g = torch.Generator().manual_seed(1000 * bn_mode + R + K + C_)
    x, da = ints(g, (R, K)), ints(g, (R, C_))
    z = ints(g, (R, C_)) + 0.5                                   # never on the ReLU boundary: gamma * z is an odd multiple of 1/8 at least
    keep = (torch.rand(R, C_, generator=g) > 0.5).to(torch.uint8)
    gamma = torch.exp2(torch.randint(-2, 3, (C_,), generator=g).float())
    d = da.double() * keep.double() * 2.0 * (z > 0).double()
    dz_ref = d * gamma.double() if bn_mode else d
    dw_ref = x.double().t() @ dz_ref
    assert float(dw_ref.abs().max()) < 2 ** 24 and float(d.sum(0).abs().max()) < 2 ** 24
    bn = dict(gamma=gamma.to(dev), beta=torch.zeros(C_, device=dev), mean=torch.zeros(C_, device=dev), invstd=torch.ones(C_, device=dev)) if bn_mode else {}
    for want_dw in (True, False):
        dz, dg, db, dbias, dw = _ops().dense_bwd(da.to(dev), z.to(dev), x.to(dev), bn_mode=bn_mode, act=1, keep=keep.to(dev), rate=0.5, want_dw=want_dw, **bn)
        torch.cuda.synchronize()
        assert torch.equal(dz.cpu(), dz_ref.float())
        if bn_mode == 0:
            assert torch.equal(dbias.cpu(), d.sum(0).float())
        if want_dw:
            assert torch.equal(dw.cpu(), dw_ref.float())
        else:
            assert dw is None


@pytest.mark.parametrize("R,K,C_,bn_mode,act,drop", [(40, 1024, 512, 1, 1, True), (33, 256, 70, 2, 1, True), (257, 9, 70, 1, 0, False),
                                                     (33, 130, 23, 0, 0, False)])
def test_dense_bwd_without_weight_gradient(dev, R, K, C_, bn_mode, act, drop):
    """dw = NULL (a frozen layer: only dz and the column sums are produced) against fp64 autograd, as test_dense_bwd_matches_autograd"""
    check_dense_bwd(dev, R, K, C_, bn_mode, act, drop, want_dw=False)


# ---------------------------------------------------------------------------------------------------------------------
# whole training steps
# ---------------------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    for profile in ("all", "classification_pretrain", "final", "heads_only"):
        for vanilla in (False, True):
            out.append((40, 136, profile, vanilla, "bf16x3"))
    out.append((33, 200, "all", False, "bf16x3"))
    for profile in ("classification_pretrain", "final"):          # bf16 + classification_pretrain: through the fused frozen segmentation head
        for precision in ("bf16x3", "bf16"):
            out.append((64, 256, profile, False, precision))
    return out


@pytest.mark.parametrize("B,N,profile,vanilla,precision", _cases())
def test_training_step_with_more_than_32_clouds(dev, B, N, profile, vanilla, precision):
    """Bd > 32: every layer teacher-forced AND the whole step against the oracle, on shape-diverse clouds with the T-Net tails damped (as
    the BASELINE configurations in tests/test_gpu_parity_configs.py, same tolerances)"""
    worst, _ = check_training_step(dev, B, N, profile, vanilla=vanilla, precision=precision, seed_params=21, seed_inputs=20260003, inputs="shapes",
                                   damp_tnet=0.1, tag=f"large-batch[{profile},vanilla={vanilla},{precision},B={B},N={N}]", **TOL[precision])
    report(f"large-batch[{profile},vanilla={vanilla},{precision},B={B},N={N}]: worst relative gradient error {worst:.3e}")


def test_both_regularisers_on_with_more_than_32_clouds(dev):
    """as test_both_regularisers_on (tests/test_gpu_parity_configs.py) at B = 40: the regularisers' gradient enters dR of both T-Nets,
    whose tails run the Bd > 32 form (dense_wgrad with the column sums for `b`)"""
    worst, m = check_training_step(dev, 40, 136, "all", precision="bf16x3", reg=True, seed_params=31, seed_inputs=32)
    sc = m.scalars.cpu()
    assert float(sc[5]) > 0 and float(sc[6]) > 0


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("vanilla", [False, True])
@pytest.mark.parametrize("profile", ["all", "final"])
@pytest.mark.parametrize("N", [1024, 200])
def test_training_step_with_a_batch_of_one(dev, N, profile, vanilla, precision):
    """B = 1: the per-cloud dense layers normalise one row with its own statistics (z - mean = 0, variance 0), so their outputs are
    relu(beta) and the gradient through them vanishes identically; teacher-forced, every line"""
    check_training_step(dev, 1, N, profile, vanilla=vanilla, precision=precision, seed_params=21, seed_inputs=20260004, inputs="shapes",
                        end_to_end=False, tag=f"batch-of-one[{profile},vanilla={vanilla},{precision},N={N}]", **TOL[precision])


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("vanilla", [False, True])
@pytest.mark.parametrize("B,N", [(16, 31), (16, 65), (3, 127)])
def test_training_step_on_short_clouds(dev, B, N, vanilla, precision):
    """N = 31 (less than one 32-row arg-max block), 65 (one row into the second 64-row panel), 127 (one row short of a statistics tile);
    teacher-forced, every line"""
    check_training_step(dev, B, N, "all", vanilla=vanilla, precision=precision, seed_params=21, seed_inputs=20260005, inputs="shapes",
                        end_to_end=False, tag=f"short-cloud[all,vanilla={vanilla},{precision},B={B},N={N}]", **TOL[precision])


# ---------------------------------------------------------------------------------------------------------------------
# step layouts
# ---------------------------------------------------------------------------------------------------------------------
def test_step_layouts_give_the_same_bits_with_more_than_32_clouds(dev):
    """the six TrainStep layouts of test_native_train_step_learns_and_graph_matches_eager (hipGraph x auxiliary stream x split optimizer)
    at B = 40: the Bd > 32 backward puts its dense weight gradients on the auxiliary stream, so the layouts must still agree bit for
    bit after a few steps from one shared start.  (That it learns is asserted at B = 8.)"""
    from pointcloudprocessing_amd.engine import TrainStep
    from pointcloudprocessing_amd.optim import KerasAdam
    from pointcloudprocessing_amd.pointnet.PointNet import PointNet, _glorot_uniform
    B, N, steps = 40, 136, 5
    g = torch.Generator().manual_seed(40)
    pc = (torch.rand(B, N, 3, generator=g) * 10).to(dev)
    y_cls = torch.randint(0, 23, (B,), generator=g, dtype=torch.int32).to(dev)
    y_seg = torch.randint(0, 12, (B, N), generator=g, dtype=torch.int32).to(dev)
    se3 = torch.eye(3).expand(B, 3, 3).contiguous().to(dev)
    finals, w0 = [], None
    for use_graph, aux, split in ((False, True, False), (True, True, False), (False, False, False), (True, False, False),
                                  (False, False, True), (True, False, True)):
        m = PointNet(23, 12, 0.0, 42, precision="bf16x3", device=dev)     # dropout 0: deterministic step
        if w0 is None:
            with torch.no_grad():       # the classification DenseLayers are unseeded, as in the reference: pin them
                for i, nme in enumerate(("mlp_cls_1.kernel", "mlp_cls_2.kernel", "mlp_cls_3.kernel")):
                    v = m._weights.view(nme)
                    v.copy_(_glorot_uniform(tuple(v.shape), 1000 + i).to(v.device))
            w0 = m.params_flat.data.clone()
        else:
            m.params_flat.data.copy_(w0)
        opt = KerasAdam(m.params_flat.data, 1e-3, 7000, 0.7)
        ts = TrainStep(m, opt, B, N, (1.0, 1.0, 1.0), use_graph=use_graph, aux=aux, split_optimizer=split)
        for _ in range(steps):
            ts(pc, y_cls, y_seg, se3)
        torch.cuda.synchronize()
        assert ts.mode == ("hipgraph" if use_graph else "eager")
        assert int(opt.iterations) == steps
        assert bool(torch.isfinite(m.params_flat.data).all())
        assert float((m.params_flat.data - w0).abs().max()) > 0
        finals.append(m.params_flat.data.clone())
    for i, f in enumerate(finals[1:]):
        assert torch.equal(finals[0], f), f"layout {i + 1} differs from layout 0"
