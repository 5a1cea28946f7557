"""The weight-gradient slabs of the six narrow per-point layers formed inside their data-gradient GEMMs
against the two-launch form.  Every check is bitwise: the fused tile stages the same values and walks the same MFMA steps in the same
order as the weight-gradient kernel, so nothing may differ.

Op level: pn_conv_bwd_data_wgrad against pn_conv_bwd_data + pn_conv_wgrad (same slab_rows) on seeded bf16 tensors, a two-source dz and
coefficients of both signs.  Step level: the same seeded trainer steps in fresh child processes with PN_WGRAD_FUSE=0 and =1."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("params", "grads", "loss_sums", "classification_output", "segmentation_output", "se3")
STEPS = 6          # two eager steps, the capture, three replays

pytestmark = pytest.mark.gpu


def _bf(t):
    return t.to(torch.bfloat16)


# B, N, K, mask, addend: the issue's four shapes (the first in fT.c1's ADD + MASK form) and the plain form on one whole chunk
CASES = [
    (2, 200, 128, True, True),      # ragged second tile of 72 rows: 64 + 8
    (3, 128, 64, True, False),      # one chunk, one whole tile
    (1, 31, 128, True, False),      # less than one chunk, one cloud
    (2, 256, 128, False, True),     # no mask, separate a operand, with addend: mlp_2_1's form
    (1, 64, 64, False, False),      # neither (never planned, but the entry accepts it)
]


@pytest.mark.parametrize("slab_rows", [64, 128])
@pytest.mark.parametrize("B,N,K,mask,add", CASES)
def test_fused_slabs_match_the_two_launches(dev, B, N, K, mask, add, slab_rows):
    from pointcloudprocessing_amd import _lib as L
    from pointcloudprocessing_amd import ops
    Cin = 64
    g = torch.Generator().manual_seed(1000 + N + K)
    dy = _bf(torch.randn(B * N, K, generator=g)).to(dev)
    zz = _bf(torch.randn(B * N, K, generator=g)).to(dev)
    ca, cb, cc = ((torch.randn(K, generator=g) * 0.5).to(dev) for _ in range(3))            # both signs
    w = (torch.randn(Cin, K, generator=g) * 0.2).to(dev)
    addend = _bf(torch.randn(B * N, Cin, generator=g)).to(dev) if add else None
    zprev = _bf(torch.randn(B * N, Cin, generator=g)).to(dev)
    msc = torch.randn(Cin, generator=g).to(dev)                                              # both signs
    msh = (torch.randn(Cin, generator=g) * 0.2).to(dev)
    prec = L.PN_PREC_BF16 | L.PN_STORE_BF16
    dz = L.operand(dy, ca=ca, cc=cc, s2=zz, cb=cb)
    # the weight gradient's operand a: ReLU(BN(Z of the previous layer)) -- the mask's tensor and coefficients -- or a plain tensor
    a = L.operand(zprev, ca=msc, cc=msh, relu=True) if mask else L.operand(zprev)
    kw = dict(addend=addend, zmask=zprev if mask else None, msc=msc if mask else None, msh=msh if mask else None)
    ref_out, ref_part = ops.conv_bwd_data(dz, w, B, N, K, Cin, prec, **kw)
    spc = (N + slab_rows - 1) // slab_rows
    # the reference slabs and all three fused results start as NaN: an element that its launch did not write cannot compare equal
    ref_slabs = torch.full((B * spc, Cin, K), float("nan"), device=dev)
    ops.check(L.lib().pn_conv_wgrad(C.byref(a), C.byref(dz), B, N, Cin, K, slab_rows, ops.ptr(ref_slabs), prec, ops.current_stream()), "pn_conv_wgrad")
    out, part, slabs = ops.conv_bwd_data_wgrad(dz, w, a, B, N, K, Cin, prec, slab_rows=slab_rows, fill=float("nan"), **kw)
    torch.cuda.synchronize()
    assert slabs.shape == ref_slabs.shape and torch.isfinite(ref_slabs).all() and float(ref_slabs.abs().max()) > 0
    assert torch.isfinite(slabs).all() and torch.isfinite(out.float()).all() and torch.isfinite(part).all()
    assert torch.equal(out, ref_out)
    assert torch.equal(part, ref_part)
    bad = [s for s in range(B * spc) if not torch.equal(slabs[s], ref_slabs[s])]
    assert not bad, (bad, float((slabs - ref_slabs).abs().max()))


def test_fused_entry_rejects_other_shapes(dev):
    from pointcloudprocessing_amd import _lib as L
    from pointcloudprocessing_amd import ops
    B, N, K = 1, 64, 64
    dy = torch.zeros(B * N, K, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(64, K, device=dev)
    co = torch.zeros(K, device=dev)
    dz = L.operand(dy, ca=co, cc=co, s2=dy, cb=co)
    prec = L.PN_PREC_BF16 | L.PN_STORE_BF16
    with pytest.raises(L.PointNetHipError):
        ops.conv_bwd_data_wgrad(dz, w, L.operand(dy), B, N, K, 64, prec, slab_rows=192)
    with pytest.raises(L.PointNetHipError):           # fp32 storage
        ops.conv_bwd_data_wgrad(dz, w, L.operand(dy), B, N, K, 64, L.PN_PREC_BF16, slab_rows=64)
    with pytest.raises(L.PointNetHipError):           # single-source dz
        ops.conv_bwd_data_wgrad(L.operand(dy), w, L.operand(dy), B, N, K, 64, prec, slab_rows=64)


def run_arm(tmp_path, tag, fuse, profile, B, N):
    out = os.path.join(str(tmp_path), f"{tag}.pt")
    env = dict(os.environ)
    env["PN_WGRAD_FUSE"] = fuse
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wgrad_fused_worker.py"), out, profile, str(B), str(N), str(STEPS)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(out, weights_only=True)


# all, B=5, N=200: slab_rows 64, two slabs per tile, a ragged last tile;  classification_pretrain, B=32, N=1024: slab_rows 128, the
# benchmark's plan
@pytest.mark.parametrize("profile,B,N", [("all", 5, 200), ("classification_pretrain", 32, 1024)])
def test_fused_plan_is_bit_identical(tmp_path, profile, B, N):
    off = run_arm(tmp_path, "off", "0", profile, B, N)
    on = run_arm(tmp_path, "on", "1", profile, B, N)
    print(f"[{profile} B={B} N={N}] fused GEMMs off {off['fused_count']} on {on['fused_count']}; planned steps {off['planned_steps']} / "
          f"{on['planned_steps']}; launch {off['mode']} / {on['mode']}")
    assert off["mode"] == on["mode"]
    assert off["fused_count"] == 0, off["fused_count"]
    assert on["planned_steps"] > 0 and on["planned_steps"] == off["planned_steps"]
    assert on["fused_count"] == 6 * on["planned_steps"], (on["fused_count"], on["planned_steps"])
    for k in KEYS:
        a, b = off[k], on[k]
        diff = float((a.double() - b.double()).abs().max()) if a.numel() else 0.0
        print(f"  {k}: max abs difference {diff:.3e} over {a.numel()} values")
        assert torch.isfinite(a).all(), k
        assert torch.equal(a, b), (k, diff)
    assert float(on["grads"].abs().max()) > 0
