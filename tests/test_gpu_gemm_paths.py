"""The row GEMMs' storage paths, exactly: the host picks the operand / epilogue storage and the kernel-copy
variant, and a whole tile of 16-bit tensors moves four columns per memory instruction through a register transposition while the ragged
last tile of a cloud keeps the element-wise form.  A wrong lane, row or column in either shows as a wrong integer here.

Operands are small integers -- exact in bf16, and every sum (the products, the statistic partials, the slabs) stays below 2^24 in
absolute terms, so it is exact in fp32 in ANY order of addition; each test asserts that bound on its own reference.  The expected values
are torch int64 arithmetic on the CPU and every comparison is for equality: outputs, statistic partials, slabs.
Shapes: B=2, N=200 (two tiles per cloud, the second ragged with 72 rows: the whole-tile and the ragged path in one launch) and B=1, N=128
(exactly one whole tile).  Through the C ABI: pn_conv_fwd, pn_conv_bwd_data, pn_conv_bwd_data_wgrad, each with bf16 and with fp32 storage.
The prepared bf16 kernel copy and the per-column constant have no argument in the C ABI: they run in the seeded model step at the end
(profile all, B=5, N=200, PN_WGRAD_FUSE=0 against 1, bit for bit), where the 64 -> 512 and the narrow segmentation layers pass through the
engine with them."""
import pytest
import torch

from test_gpu_wgrad_fused import KEYS, run_arm

pytestmark = pytest.mark.gpu

SHAPES = [(2, 200), (1, 128)]
LIMIT = 1 << 24


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)


def _pick(g, n, values):
    return torch.tensor(values, dtype=torch.int64)[torch.randint(0, len(values), (n,), generator=g)]


def _sparse_kernel(g, rows, cols):
    """entries in {-1, 0, 1}, about a quarter of them set: keeps |product sums| small enough for exact squares"""
    return _ints(g, (rows, cols), -1, 1) * (torch.rand(rows, cols, generator=g) < 0.25)


def _act(t, s16, dev):
    return t.to(torch.bfloat16 if s16 else torch.float32).to(dev)


def _tile_sums(v, w2, B, N):
    """per 128-row tile of each cloud: (sum v, sum v * w2) and the absolute bound of the second"""
    C_ = v.shape[1]
    tpc = (N + 127) // 128
    part = torch.zeros(B * tpc, 2, C_, dtype=torch.int64)
    bound = 0
    v3, w3 = v.view(B, N, C_), w2.view(B, N, C_)
    for b in range(B):
        for t in range(tpc):
            rows = slice(t * 128, min(N, (t + 1) * 128))
            part[b * tpc + t, 0] = v3[b, rows].sum(0)
            part[b * tpc + t, 1] = (v3[b, rows] * w3[b, rows]).sum(0)
            bound = max(bound, int((v3[b, rows] * w3[b, rows]).abs().sum(0).max()))
    return part, bound


def _check(out, part, v, w2, B, N, s16):
    exp_part, bound = _tile_sums(v, w2, B, N)
    assert bound < LIMIT and int(v.abs().max()) < LIMIT, bound
    exp_out = v.float().to(torch.bfloat16) if s16 else v.float()
    assert out.dtype == exp_out.dtype
    bad = (out.cpu() != exp_out).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), out.cpu()[tuple(bad[0])].item(), exp_out[tuple(bad[0])].item())
    assert torch.equal(part.cpu(), exp_part.float()), (part.cpu() - exp_part.float()).abs().max().item()


@pytest.mark.parametrize("s16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K,C_", [(64, 64), (64, 128)])
@pytest.mark.parametrize("B,N", SHAPES)
def test_forward_is_exact(dev, B, N, K, C_, s16):
    from pointcloudprocessing_amd import _lib as L
    from pointcloudprocessing_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + K + C_)
    x = _ints(g, (B * N, K), 0, 1)
    ca, cc = _pick(g, K, [1, 2]), _pick(g, K, [-1, 0])
    w = _sparse_kernel(g, K, C_)
    bias = _ints(g, (B, C_), -2, 2)
    staged = (x * ca + cc).clamp(min=0)                                  # lazy BatchNorm + ReLU, in {0, 1, 2}
    v = staged @ w + bias.repeat_interleave(N, 0)
    op = L.operand(_act(x, s16, dev), ca=ca.float().to(dev), cc=cc.float().to(dev), relu=True)
    prec = L.PN_PREC_BF16 | (L.PN_STORE_BF16 if s16 else 0)
    out, part = ops.conv_fwd(op, w.float().to(dev), B, N, K, C_, prec, cloud_bias=bias.float().to(dev))
    torch.cuda.synchronize()
    _check(out, part, v, v, B, N, s16)


def _dz(g, M, K, two, s16, dev):
    from pointcloudprocessing_amd import _lib as L
    dy, ca, cc = _ints(g, (M, K), -1, 1), _pick(g, K, [1, 2]), _pick(g, K, [-1, 0, 1])
    dz = dy * ca + cc
    kw = {}
    if two:                                                                # dz = ca dy + cb z + cc
        z, cb = _ints(g, (M, K), -1, 1), _pick(g, K, [-1, 1])
        dz = dz + z * cb
        kw = dict(s2=_act(z, s16, dev), cb=cb.float().to(dev))
    return dz, L.operand(_act(dy, s16, dev), ca=ca.float().to(dev), cc=cc.float().to(dev), **kw)


# 128 -> 64 with the two-source dz; 128 -> 128 with addend and mask (the max-pooled layers' data gradient)
@pytest.mark.parametrize("s16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K,C_,two,extras", [(128, 64, True, False), (128, 128, False, True)])
@pytest.mark.parametrize("B,N", SHAPES)
def test_data_gradient_is_exact(dev, B, N, K, C_, two, extras, s16):
    from pointcloudprocessing_amd import _lib as L
    from pointcloudprocessing_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + K + C_ + 7)
    M = B * N
    dz, op = _dz(g, M, K, two, s16, dev)
    w = _sparse_kernel(g, C_, K)                                           # the layer's (cin, cout) kernel
    v = dz @ w.t()
    w2, kw = v, {}
    if extras:
        addend, zm = _ints(g, (M, C_), -3, 3), _ints(g, (M, C_), -2, 2)
        msc, msh = _pick(g, C_, [-1, 1, 2]), _pick(g, C_, [-1, 0, 1])
        v = torch.where(zm * msc + msh > 0, v + addend, torch.zeros_like(v))
        w2 = zm
        kw = dict(addend=_act(addend, s16, dev), zmask=_act(zm, s16, dev), msc=msc.float().to(dev), msh=msh.float().to(dev))
    prec = L.PN_PREC_BF16 | (L.PN_STORE_BF16 if s16 else 0)
    out, part = ops.conv_bwd_data(op, w.float().to(dev), B, N, K, C_, prec, **kw)
    torch.cuda.synchronize()
    _check(out, part, v, w2, B, N, s16)


# the fused data + weight gradient (bf16 storage only): outputs, partials and slabs
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("B,N", SHAPES)
def test_fused_data_and_weight_gradient_is_exact(dev, B, N, K):
    from pointcloudprocessing_amd import _lib as L
    from pointcloudprocessing_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + K + 11)
    M, Cin, rows = B * N, 64, 64
    dz, op = _dz(g, M, K, True, True, dev)
    w = _sparse_kernel(g, Cin, K)
    zprev = _ints(g, (M, Cin), -2, 2)
    msc, msh = _pick(g, Cin, [-1, 1, 2]), _pick(g, Cin, [-1, 0, 1])
    a = (zprev * msc + msh).clamp(min=0)                                   # the slab's operand a: ReLU(BN(Z of the previous layer))
    v = torch.where(zprev * msc + msh > 0, dz @ w.t(), torch.zeros(M, Cin, dtype=torch.int64))
    a_op = L.operand(_act(zprev, True, dev), ca=msc.float().to(dev), cc=msh.float().to(dev), relu=True)
    out, part, slabs = ops.conv_bwd_data_wgrad(op, w.float().to(dev), a_op, B, N, K, Cin, L.PN_PREC_BF16 | L.PN_STORE_BF16, slab_rows=rows,
                                               zmask=_act(zprev, True, dev), msc=msc.float().to(dev), msh=msh.float().to(dev), fill=float("nan"))
    torch.cuda.synchronize()
    _check(out, part, v, zprev, B, N, True)
    spc = (N + rows - 1) // rows
    exp = torch.zeros(B * spc, Cin, K, dtype=torch.int64)
    for b in range(B):
        for s in range(spc):
            r = slice(b * N + s * rows, b * N + min(N, (s + 1) * rows))
            exp[b * spc + s] = a[r].t() @ dz[r]
    assert int(exp.abs().max()) < LIMIT
    assert torch.equal(slabs.cpu(), exp.float())


def test_model_step_all_profile_is_bit_identical_across_fuse_arms(tmp_path):
    off = run_arm(tmp_path, "off", "0", "all", 5, 200)
    on = run_arm(tmp_path, "on", "1", "all", 5, 200)
    assert off["mode"] == on["mode"] and off["fused_count"] == 0 and on["fused_count"] == 6 * on["planned_steps"] > 0
    for k in KEYS:
        assert torch.isfinite(off[k]).all(), k
        assert torch.equal(off[k], on[k]), k
    assert float(on["grads"].abs().max()) > 0
