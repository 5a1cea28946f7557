"""The carried launches (a max-pooled layer's backward preparation in the dense chain's last launch, the
d(R_64) slab reduction behind the d(A_12) row tiles) against the launch-by-launch plan: the same seeded steps in fresh child processes
with the plan's switches off and on must give the same bits -- the arithmetic is the same bodies in the same order, only the launch
that runs them differs -- and the switched-on arm must really have taken the carried forms."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("PN_PREP_CARRY", "PN_DR64_RIDE")
KEYS = ("params", "grads", "loss_sums", "classification_output", "segmentation_output", "se3")
STEPS = 6          # two eager steps, the capture, three replays


def run_arm(tmp_path, tag, on, profile, B, N):
    out = os.path.join(str(tmp_path), f"{tag}.pt")
    env = dict(os.environ)
    for s in SWITCHES:
        env[s] = "1" if on else "0"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "carry_worker.py"), out, profile, str(B), str(N), str(STEPS)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(out, weights_only=True)


@pytest.mark.gpu
@pytest.mark.parametrize("profile,B,N", [("classification_pretrain", 32, 1024), ("all", 5, 200)])
def test_carried_plan_is_bit_identical(tmp_path, profile, B, N):
    off = run_arm(tmp_path, "off", False, profile, B, N)
    on = run_arm(tmp_path, "on", True, profile, B, N)
    print(f"[{profile} B={B} N={N}] plan counts off {off['plan_count']} on {on['plan_count']}; launch {off['mode']} / {on['mode']}")
    assert off["mode"] == on["mode"]
    # the switched-off arm ran the launch-by-launch plan, the other one the carried forms: three preparations (the two T-Nets' and
    # mlp_2_3's) and one d(R_64) reduction per planned step; index 1 is retired
    assert off["plan_count"] == [0, 0, 0], off["plan_count"]
    assert on["plan_count"][2] > 0 and on["plan_count"][0] == 3 * on["plan_count"][2] and on["plan_count"][1] == 0, on["plan_count"]
    for k in KEYS:
        a, b = off[k], on[k]
        diff = float((a.double() - b.double()).abs().max()) if a.numel() else 0.0
        print(f"  {k}: max abs difference {diff:.3e} over {a.numel()} values")
        assert torch.isfinite(a).all(), k
        assert torch.equal(a, b), (k, diff)
    assert float(on["grads"].abs().max()) > 0
