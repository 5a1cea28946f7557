#!/usr/bin/env python3
"""Where a workgroup of the row GEMMs spends its cycles: runs the PN_GEMM_DBG=16 instantiations (the product tile + s_memtime readings
of wave 0 at its phase boundaries, summed per phase and left over the tile's first eight statistic partials) at the step's shape
(B=32, N=1024, bf16 operands and storage) and prints, per kernel, the median over the workgroups of every phase in shader cycles and as a
share of the workgroup's span.  Phases: operands requested (every issue), staged (conversion + LDS writes + barrier), MFMAs (+ barrier),
the slab operand's image, epilogue (addend / mask loads, output stores, statistics), slabs, outstanding stores drained.
In the two kinds that stage the prepared bf16 kernel copy the stamped launch takes that copy through `w`."""
import json
import os
import sys

import numpy as np
import torch

os.environ["PN_GEMM_DBG"] = "16"      # read once, at the first launch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudprocessing_amd import _lib, ops   # noqa: E402

PHASES = ("requested", "staged", "mfma", "slab_operand", "epilogue", "slabs", "drain")
dev = torch.device("cuda:0")
B, N = 32, 1024
M = B * N
PREC = _lib.PREC["bf16"]
g = torch.Generator().manual_seed(6)


def act(c):
    return torch.randn(M, c, generator=g).to(dev).to(torch.bfloat16)


def vec(c, pos=False):
    return ((torch.rand(c, generator=g) + 0.5) if pos else torch.randn(c, generator=g) * 0.3).to(dev)


def report(name, launch):
    for _ in range(3):
        part = launch()
    torch.cuda.synchronize()
    st = part.view(torch.int32).reshape(part.shape[0], -1)[:, :8].cpu().numpy().astype(np.int64) & 0xffffffff
    med = np.median(st, axis=0)
    span = float(med[7])
    print(json.dumps({"kernel": name, "B": B, "N": N, "workgroups": int(st.shape[0]),
                      "phase_cycles_median": {p: int(med[i]) for i, p in enumerate(PHASES)},
                      "phase_share_of_span": {p: round(float(med[i]) / span, 3) for i, p in enumerate(PHASES)},
                      "wg_span_median": int(span), "wg_span_max": int(st[:, 7].max()),
                      "staging_epilogue_slab_share": round(float(med[1] + med[3] + med[4] + med[5]) / span, 3)}), flush=True)


# the 64 -> 64 forward: lazy BatchNorm + ReLU operand, the transposed kernel copy
w64 = (torch.randn(64, 64, generator=g) / 8).to(dev)
x_op = _lib.operand(act(64), ca=vec(64, True), cc=vec(64), relu=True)
wt16 = ops.weights_copy16(w64)[1]
report("gemm_kernel<128,64,1,FWD> 64->64 forward", lambda: ops.conv_fwd(x_op, wt16, B, N, 64, 64, PREC)[1])

# the max-pooled layers' data gradient: 128 x 128, fp32 kernel (Pm), addend and mask
wpm = (torch.randn(128, 128, generator=g) / 11).to(dev)
d_op = _lib.operand(act(128), ca=vec(128, True), cc=vec(128), relu=True)
add, zm, msc, msh = act(128), act(128), vec(128, True), vec(128)
report("gemm_kernel<128,128,1,BWD,addend,mask> 128->128 data gradient",
       lambda: ops.conv_bwd_data(d_op, wpm, B, N, 128, 128, PREC, addend=add, zmask=zm, msc=msc, msh=msh)[1])

# the fused data + weight gradient of a narrow layer: two-source dz, mask, the kernel copy as it is
for K in (64, 128):
    wk = (torch.randn(64, K, generator=g) / 8).to(dev)
    w16 = ops.weights_copy16(wk)[0]
    dz_op = _lib.operand(act(K), ca=vec(K, True), cc=vec(K), s2=act(K), cb=vec(K))
    a_op = _lib.operand(act(64), ca=vec(64, True), cc=vec(64), relu=True)
    zm64, msc64, msh64 = act(64), vec(64, True), vec(64)
    report(f"gemm_bwd_wgrad_kernel<false,true> {K}->64 data + weight gradient",
           lambda: ops.conv_bwd_data_wgrad(dz_op, w16, a_op, B, N, K, 64, PREC, slab_rows=128, zmask=zm64, msc=msc64, msh=msh64)[1])
