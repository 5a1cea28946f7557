"""The argument checks of the training launchers, through their C ABI entries and without a GPU: every row below must be refused with
PN_ERR_INVALID_ARGUMENT and the recorded text before any HIP call.  The pointers are fake and never dereferenced, so the module skips
itself where a GPU is present: a row that slipped through must fail here as PN_ERR_LAUNCH, never start a kernel on such addresses.
The texts were recorded from the launchers while each still carried its own copy of these checks; they are what a caller of
pn_last_error() sees, whichever function now holds the check."""
import ctypes as C

import pytest
import torch

from pointcloudprocessing_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: only where no kernel can start")

FAKE = 0x1000                # 16-byte aligned, never dereferenced
P = C.c_void_p(FAKE)
B, N, K, CH = 2, 64, 128, 1024          # the max-pool entries
R, DK, DC = 4, 64, 32                   # the dense entries


def operand(**kw):
    f = dict(s1=FAKE, s2=None, ca=None, cb=None, cc=None, ld=K, lo=0.0, h16=0)
    f.update(kw)
    return _lib.pn_operand(**f)


def max_resolve(x=None, wf_lo=P, K=K, C_=CH, prec=_lib.PN_PREC_BF16):
    return ("pn_max_resolve", [C.byref(x or operand()), P, wf_lo, P, B, N, K, C_, P, prec, None])


def maxbwd_scatter(q=P, K=K):
    return ("pn_maxbwd_scatter", [P, P, P, q, B, N, K, CH, P, 0, None])


def bn_finalize(gamma=P, C_=CH):
    return ("pn_bn_finalize", [P, 4, C_, B * N, gamma, P, P, P, 0.9, 1e-3, 1, 1, P, P, P, P, None])


def panel_finalize(g=P):
    return ("pn_panel_finalize", [P, P, P, P, P, P, _lib.PN_PREC_BF16, B, N, K, CH, P, P, P, P, 0.9, 1e-3, 1, 1, P, P, P, P, g, P, P, None])


def dense_layer(C_=DC, gamma=P, bn_mode=0, z_out=P):
    return ("pn_dense_layer", [P, DK, P, C_, 0, R, DK, C_, P, P, P, gamma, P, P, P, 0.9, 1e-3, bn_mode, 1, None, 1.0, z_out, P, P, P, None])


def dense_bwd(R=R, x=P, mean=P, bn_mode=0, dw=None):
    return ("pn_dense_bwd", [P, P, x, DK, R, DK, DC, P, P, mean, P, bn_mode, 1, None, 1.0, P, P, P, P, dw, None])


def dense_bwd_step(R=R, **kw):
    f = dict(z=FAKE, gamma=FAKE, beta=FAKE, mean=FAKE, invstd=FAKE, keep=None, keep_scale=1.0, bn_mode=0, act=1, dz=FAKE, dgamma=None,
             dbeta=None, dbias=None)
    f.update(kw)
    return ("pn_dense_bwd_step", [P, DK, P, DK, R, DK, DC, P, P, P, C.byref(_lib.pn_dense_tail(**f)), None])


RESOLVE_SHAPES = b"K must be a multiple of 16, at most 128, C a multiple of 32"
BN_BWD = b"BatchNormalization needs gamma/beta/mean/invstd"
CASES = {
    "max_resolve-K144": (max_resolve(K=144), RESOLVE_SHAPES),
    "max_resolve-C1000": (max_resolve(C_=1000), RESOLVE_SHAPES),
    "max_resolve-x3-without-lo": (max_resolve(prec=_lib.PN_PREC_BF16X3, wf_lo=None), b"bad prec / missing lo weights"),
    "max_resolve-h16-ld132": (max_resolve(x=operand(h16=1, ld=132)), b"16-bit rows need ld % 8 == 0"),
    "max_resolve-s2": (max_resolve(x=operand(s2=FAKE)), b"null pointer"),
    "max_resolve-s1-unaligned": (max_resolve(x=operand(s1=0x1004)), b"operand alignment"),
    "maxbwd_scatter-K48": (maxbwd_scatter(K=48), b"K must be a multiple of 32, at most 128 (K=48)"),
    "maxbwd_scatter-q-null": (maxbwd_scatter(q=None), b"null pointer"),
    "bn_finalize-gamma-null": (bn_finalize(gamma=None), b"null pointer"),
    "bn_finalize-C0": (bn_finalize(C_=0), b"C must be positive"),
    "panel_finalize-g-null": (panel_finalize(g=None), b"null pointer"),
    "dense_layer-bn-without-gamma": (dense_layer(bn_mode=1, gamma=None), b"BatchNormalization needs gamma/beta/moving statistics"),
    "dense_layer-C8224": (dense_layer(C_=8224), b"C=8224 needs more than 256 counters"),
    "dense_layer-z_out-null": (dense_layer(z_out=None), b"bad arguments"),
    "dense_bwd-R4-dw-without-x": (dense_bwd(dw=P, x=None), b"the weight gradient needs the layer input"),
    "dense_bwd-R4-bn-without-mean": (dense_bwd(bn_mode=1, mean=None), BN_BWD),
    "dense_bwd-R40-bn-without-mean": (dense_bwd(R=40, bn_mode=1, mean=None), BN_BWD),
    "dense_bwd_step-tail-R40": (dense_bwd_step(R=40), b"the backward tail needs R <= 32 (R=40)"),
    "dense_bwd_step-tail-bn-without-gamma": (dense_bwd_step(bn_mode=1, gamma=None), BN_BWD),
    "dense_bwd_step-tail-z-null": (dense_bwd_step(z=None), b"null pointer in the tail"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_bad_argument_is_refused_with_its_text(case):
    (entry, args), text = CASES[case]
    L = _lib.lib()
    rc = getattr(L, entry)(*args)
    assert rc == -1, (rc, L.pn_last_error())          # PN_ERR_INVALID_ARGUMENT
    assert text in L.pn_last_error(), L.pn_last_error()


def test_the_valid_arguments_pass_the_checks():
    """the base of every row above is itself accepted: without a GPU it gets as far as the launch, which fails (PN_ERR_LAUNCH), so each
    row is refused for its one bad argument and nothing else"""
    L = _lib.lib()
    for entry, args in (max_resolve(), maxbwd_scatter(), bn_finalize(), panel_finalize(), dense_layer(), dense_bwd(), dense_bwd(R=40),
                        dense_bwd_step()):
        assert getattr(L, entry)(*args) == -2, (entry, L.pn_last_error())
