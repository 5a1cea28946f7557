"""Every arm of the plan and every held-back kernel that one environment variable can reach, each in a fresh child
process (tests/plan_arm_worker.py: the switches are read once per process), one child at a time.

What an arm is held to.  Every training arm must pass parity_harness.check_training_step on every case -- each layer teacher-forced in
fp64 from the GPU's own stored inputs, and the whole step against the oracle, with the project's tolerances -- exactly as the default
plan does in tests/test_gpu_large_batch.py: the reference judges the arm, never the default arm's numbers.  On top of that an arm whose
arithmetic is the default plan's (only the launch that runs it differs) must reproduce the default arm bit for bit, and an arm has a
WITNESS where the plan offers one: an observable that shows the switch reached the process and changed the path.  The difference of
every arm's gradients from the default arm's is printed and written to the parity report (parity_harness.report): information for whoever uses the
arm as a yardstick, not a threshold.

The default arm runs once per mode with no PN_* variable in its environment; if IT fails a case, the case list is invalid and the
fixture says so.

Slab-count arms: what wgrad_slab_rows (pn_model.hip) returns, computed on the CPU (tests/test_cpu_plan_arms.py asserts these), as
(rows per slab, slabs per cloud) for the job shapes 64x64 / 64x128 / 128x128 | 64x512 | 512x256 | 256x128:
    default (256 / 128)  B=5  N=200   (64, 4) | (64, 4)  | (64, 4)  | (64, 4);   B=40 N=136  (64, 3) | (128, 2) | (192, 1) | (64, 3)
    PN_WGRAD_TARGET*=8   B=5  N=200   (128, 2): a two-tile slab and a ragged second slab of 72 rows | (256, 1) | (256, 1) | (256, 1)
                         B=40 N=136   (192, 1) for every shape: three tiles, the last of 8 rows
                         B=2  N=2100  (576, 4): nine tiles, the last slab ragged (372 rows: five tiles and one of 52 rows) | (2112, 1) |
                                      (2112, 1) | (1088, 2): a ragged second slab of 1012 rows   [default: (64, 33) | (128, 17) | (192, 11) | (64, 33)]
    PN_WGRAD_TARGET*=1   B=5  N=200   (256, 1) for every shape: the whole cloud in one slab
and the Pm job of PN_PM_IN_PREP=0 (1024 "rows"): (64, 16) by default, (128, 8) at 8, (1024, 1) at 1.  The 64-channel layers' slabs
are formed inside their data-gradient GEMMs in the bf16 mode when rows is 64 or 128 (pn_model_wgrad_fused_count): at 8 and B = 5 that
is the 128-row form, at 1 the plan falls back to the weight-gradient launches -- the one-slab arm's witness.

Dense-split arms (PN_DENSE_KSPLIT = k per split; pn_dense.hip: launch_dense picks DEPTH from the 64-k steps of a split, 2 / 4 / 8 for
up to 2 / 4 / more).  The model's vector-load instantiations of dense_layer_kernel<TRANS, DEPTH, VEC> at K = 1024 / 512 / 256:
    default (128)  forward <false,2,true> at every K with splits of 128 (8 / 4 / 2 of them), <false,4,true> only as the single split of
                   a one-column-block layer (K = 256: the logits, the T-Nets' 256 -> K*K); backward <true,2,true> at K = 512 / 256;
    256            forward K = 1024: 4 splits <false,4,true>; 512: 2 splits <false,4,true>; 256: one split <false,4,true>, no ticket;
                   backward K = 512: 2 splits <true,4,true>; 256: one split <true,4,true>;
    512            forward K = 1024: 2 splits <false,8,true>; 512: one split <false,8,true>; 256: one split <false,4,true>;
                   backward K = 512: one split <true,8,true>; 256: one split <true,4,true>;
    1024           forward K = 1024: one split <false,8,true> (two rounds of 8 steps); 512, 256 as at 512; backward as at 512.
The default plan never runs <false,8,true>, <true,4,true>, <true,8,true>, nor <false,4,true> with a ticket or on more than one column
block; the op-level checks (mode 'dense_ops') add R > 32 and the odd shapes (these stay on <.,2,false>, whose split lengths change).
With splits longer than 128 the carried preparation launch (dense_prep_carry_kernel, built for DEPTH 2) does not fit and the plan
falls back to maxbwd_prep_resolve: pn_model_plan_count(0) stays 0 -- these arms' witness.

Wide-tile arm: only mlp_seg_2 (512 -> 256, 16-bit operands) takes wgrad_batch_kernel<128,256,1,.>; conv_wgrad_batch's key() excludes
the split-operand mode, hence bf16 only.  It has no witness (no counter or workspace entry tells the tile shapes apart).
"""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

from parity_harness import report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "plan_arm_worker.py")
TIMEOUT = 600          # as tests/test_gpu_carry.py

PRECISIONS = ("bf16x3", "bf16")
SMALL, SMALL_VANILLA, LARGE = (5, 200, "all", False), (5, 200, "all", True), (40, 136, "all", False)


def train_cases(shapes=(SMALL, SMALL_VANILLA, LARGE), precisions=PRECISIONS):
    return [list(s) + [p] for s in shapes for p in precisions]


# two long clouds with a ragged end (52 rows in the last 64-row tile of the max-pool backward's scatter), the farthest points of each
# cloud moved into that tile (parity_harness.farthest_point_last), teacher-forced only (two clouds): the default arm runs
# maxbwd_scatter_reduce<2>, PN_PM_IN_PREP=0 maxbwd_scatter<2> with q inside the plan, the few-slab arm 576-row slabs with a ragged last one
LONG_RAGGED = [[2, 2100, "all", False, p, "ragged"] for p in PRECISIONS]


# (B, N, vanilla): whole 128-row tiles; a last tile of 72 rows (rows in both 64-row halves); a last tile whose second half is empty;
# one partial tile, first half only; the vanilla model; and of tests/inference_cases.py one partial tile shorter than a 32-row block and
# a tile whose second half holds one row
SEGHEAD_CASES = [[2, 256, False], [3, 200, False], [2, 192, False], [1, 50, False], [2, 200, True], [5, 31, False], [3, 65, False]]
# the last three, of tests/inference_cases.py: one ragged slot shorter than a 32-row block; a single row; more than 128 clouds (vanilla)
INFER_CASES = [[3, 200, False], [3, 200, True], [2, 4099, False], [5, 31, False], [1, 1, False], [130, 40, True]]

# arm -> (environment, cases); the switches named here are the first list of tests/test_cpu_plan_arms.py
TRAIN_ARMS = {
    "pm_own_launch": ({"PN_PM_IN_PREP": 0}, train_cases() + LONG_RAGGED),
    "pm_own_launch_128_tiles": ({"PN_PM_IN_PREP": 0, "PN_PM_SMALL": 0}, train_cases((SMALL, SMALL_VANILLA))),
    "dense_wgrad_own_launch": ({"PN_DENSE_RIDE": 0}, train_cases()),
    "few_slabs": ({"PN_WGRAD_TARGET": 8, "PN_WGRAD_TARGET_GRAM": 8}, train_cases() + LONG_RAGGED),
    "one_slab": ({"PN_WGRAD_TARGET": 1, "PN_WGRAD_TARGET_GRAM": 1}, train_cases((SMALL,))),
    "dense_whole_k": ({"PN_DENSE_KSPLIT": 1024}, train_cases()),
    "dense_split_256": ({"PN_DENSE_KSPLIT": 256}, train_cases((SMALL,))),
    "dense_split_512": ({"PN_DENSE_KSPLIT": 512}, train_cases((SMALL,))),
    "wide_wgrad_tiles": ({"PN_WGRAD_WIDE": 1}, train_cases(precisions=("bf16",))),
}
SEGHEAD_ARM = {"PN_SEGHEAD_MB": 4}
INFER_ARM = {"PN_CHAIN_FUSE": 0}
INFER_WITNESS = "m22.Z"      # mlp_2_2's stored output: written by the layer-by-layer plan, kept on chip by the chain kernel
KEYS = ("grads", "classification_output", "segmentation_output", "se3", "loss_sums")


def run_arm(tmp, tag, env_switches, mode, cases):
    """one child; returns its records.  A child that faulted, aborted or timed out fails the calling test at once."""
    out, cj = os.path.join(str(tmp), tag + ".pt"), os.path.join(str(tmp), tag + ".json")
    with open(cj, "w") as f:
        json.dump(cases, f)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PN_")}
    env.update({k: str(v) for k, v in env_switches.items()})
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, WORKER, out, mode, cj], env=env, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"arm {tag} {env_switches}: the child did not end within {TIMEOUT} s", pytrace=False)
    wall = time.time() - t0
    line = f"plan-arm child {tag} ({mode}, {env_switches or 'default'}, {len(cases) or 'op-level'} cases): {wall:.1f} s wall, exit {r.returncode}"
    print(line)
    report(line)
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.fail(f"arm {tag} {env_switches}: the child died (exit {r.returncode})\n" + r.stderr[-3000:], pytrace=False)
    assert r.returncode in (0, 1) and os.path.exists(out), (tag, r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    return torch.load(out, weights_only=True)


def failures(records):
    return [(rec["case"], rec["error"]) for rec in records if rec["error"]]


def default_arm(tmp_path_factory, mode, cases):
    recs = run_arm(tmp_path_factory.mktemp("default_" + mode), "default", {}, mode, cases)
    bad = failures(recs)
    if bad:
        pytest.fail(f"the case list of mode '{mode}' is invalid: the DEFAULT plan fails {[c for c, _ in bad]}\n" + bad[0][1], pytrace=False)
    return {json.dumps(rec["case"]): rec for rec in recs}


@pytest.fixture(scope="module")
def default_train(dev, tmp_path_factory):
    return default_arm(tmp_path_factory, "train", train_cases() + LONG_RAGGED)


@pytest.fixture(scope="module")
def default_seghead(dev, tmp_path_factory):
    return default_arm(tmp_path_factory, "seghead", SEGHEAD_CASES)


@pytest.fixture(scope="module")
def default_infer(dev, tmp_path_factory):
    return default_arm(tmp_path_factory, "infer", INFER_CASES)


@pytest.fixture(scope="module")
def default_dense_ops(dev, tmp_path_factory):
    return default_arm(tmp_path_factory, "dense_ops", [])


@pytest.fixture(scope="module")
def train_arm_records(dev, tmp_path_factory):
    """the records of the training arms run so far (the 128-tile Pm arm is compared with the Pm arm, not with the default)"""
    cache = {}

    def get(arm):
        if arm not in cache:
            env, cases = TRAIN_ARMS[arm]
            cache[arm] = {json.dumps(rec["case"]): rec for rec in run_arm(tmp_path_factory.mktemp(arm), arm, env, "train", cases)}
        return cache[arm]
    return get


def difference(tag, arm, base):
    """largest absolute and relative difference of the gradients per case (printed and reported; not a threshold); True: every bit equal"""
    same = True
    for k, rec in arm.items():
        a, b = rec["grads"].double(), base[k]["grads"].double()
        d = float((a - b).abs().max())
        eq = all(torch.equal(rec[q], base[k][q]) for q in KEYS)
        same = same and eq
        line = (f"plan-arm {tag} case {k}: gradients differ by {d:.3e} abs, {d / (float(b.abs().max()) + 1e-300):.3e} of the largest; "
                f"grads / outputs / loss sums {'bit-identical' if eq else 'NOT bit-identical'}; plan_count {rec['plan_count']} "
                f"wgrad_fused {rec['wgrad_fused_count']} pm_slabs {rec['pm_slabs']}")
        print(line)
        report(line)
    return same


@pytest.mark.parametrize("arm", list(TRAIN_ARMS))
def test_training_arm_meets_the_oracle(default_train, train_arm_records, arm):
    """every case of the arm passes check_training_step (the acceptance of every arm); then the arm's relation to the default arm and its
    witness, as the module docstring has them"""
    env, cases = TRAIN_ARMS[arm]
    recs = train_arm_records(arm)
    bad = failures(recs.values())
    assert not bad, f"arm {arm} {env} fails the oracle on {[c for c, _ in bad]}\n" + bad[0][1]
    assert sorted(recs) == sorted(json.dumps(c) for c in cases)
    base = train_arm_records("pm_own_launch") if arm == "pm_own_launch_128_tiles" else default_train
    same = difference(f"{arm} vs {'pm_own_launch' if base is not default_train else 'default'}", recs, base)
    for k, rec in recs.items():
        B, N, _, vanilla, precision = rec["case"][:5]
        d = default_train[k]
        # the default arm's own witnesses: Pm from the preparation workgroups, which the dense chain's last launch carries up to 32 clouds
        assert d["pm_slabs"] == "finite", (k, d["pm_slabs"])
        assert (d["plan_count"][0] == 0) if B > 32 else (d["plan_count"][0] > 0), (k, d["plan_count"])
        if arm.startswith("pm_own_launch"):
            assert rec["pm_slabs"] == "poison", (k, rec["pm_slabs"])               # nothing wrote the preparation's Pm slabs
            assert rec["plan_count"][0] == 0, (k, rec["plan_count"])                # and no launch carried the preparation
        if arm.startswith("dense_"):
            assert rec["pm_slabs"] == "finite", (k, rec["pm_slabs"])
        if arm in ("dense_whole_k", "dense_split_256", "dense_split_512"):
            assert rec["plan_count"][0] == 0, (k, rec["plan_count"])                # the carried launch is built for 128-k splits only
        if precision == "bf16":
            assert d["wgrad_fused_count"] > 0, (k, d["wgrad_fused_count"])          # 64-row slabs formed inside the data-gradient GEMMs
            long_slabs = B > 32 or N >= 2048                                         # few_slabs: 192-row slabs / 576 rows and more
            if arm == "one_slab" or (arm == "few_slabs" and long_slabs):
                assert rec["wgrad_fused_count"] == 0, (k, rec["wgrad_fused_count"])   # 256- / 192-row slabs: the launches of their own
            if arm == "few_slabs" and not long_slabs:
                assert rec["wgrad_fused_count"] > 0, (k, rec["wgrad_fused_count"])     # 128-row slabs: still fused
    if arm in ("dense_wgrad_own_launch", "pm_own_launch_128_tiles"):
        assert same, f"arm {arm} {env} runs the same arithmetic as its base arm and must keep every bit"
    report(f"plan-arm {arm} {env}: oracle passed on {len(recs)} cases; {'bit-identical to' if same else 'differs from'} its base arm")


@pytest.mark.parametrize("ksplit", [1024, 512, 256])
def test_dense_ops_under_a_dense_split(default_dense_ops, tmp_path, ksplit):
    """the dense layers' op-level checks of tests/test_gpu_ops.py (fp64 references, their own parametrisations and tolerances) with the
    contraction split every `ksplit` k: R > 32, ragged C and K, the backward chain step"""
    recs = run_arm(tmp_path, f"dense_ops_{ksplit}", {"PN_DENSE_KSPLIT": ksplit}, "dense_ops", [])
    assert len(recs) == len(default_dense_ops) > 0
    bad = failures(recs)
    assert not bad, f"PN_DENSE_KSPLIT={ksplit} fails {[c for c, _ in bad]}\n" + bad[0][1]


def test_segmentation_head_128_row_tiles_equal_the_64_row_form(default_seghead, tmp_path):
    """PN_SEGHEAD_MB=4 runs seg_head_fused_kernel<4,.>: in its own process it must equal the layer-by-layer plan (the assertions of
    test_fused_frozen_segmentation_head_equals_layer_by_layer), and across processes the 64-row form bit for bit -- per row both are the
    same arithmetic; the loss / accuracy sums are grouped per 128 instead of 64 rows and agree to rounding"""
    recs = run_arm(tmp_path, "seghead_mb4", SEGHEAD_ARM, "seghead", SEGHEAD_CASES)
    bad = failures(recs)
    assert not bad, f"{SEGHEAD_ARM}: the 128-row form differs from the layer-by-layer plan on {[c for c, _ in bad]}\n" + bad[0][1]
    assert len(recs) == len(SEGHEAD_CASES)
    for rec in recs:
        d = default_seghead[json.dumps(rec["case"])]
        for a, b in zip(rec["inference"] + rec["training"] + [rec["grads"]], d["inference"] + d["training"] + [d["grads"]]):
            assert torch.isfinite(a).all() and torch.equal(a, b), rec["case"]
        assert float(rec["grads"].abs().max()) > 0
        assert torch.allclose(rec["loss_sums"], d["loss_sums"], rtol=1e-5, atol=1e-5), (rec["case"], rec["loss_sums"].tolist(), d["loss_sums"].tolist())


def test_inference_without_the_chain_kernel_keeps_every_bit(default_infer, tmp_path):
    """PN_CHAIN_FUSE=0: the three launches the chain kernel replaces.  Same outputs bit for bit; the witness is the workspace entry
    INFER_WITNESS, which only the layer-by-layer plan writes (the workspace is poisoned before the call)."""
    recs = run_arm(tmp_path, "infer_unfused", INFER_ARM, "infer", INFER_CASES)
    assert not failures(recs) and len(recs) == len(INFER_CASES)
    for rec in recs:
        d = default_infer[json.dumps(rec["case"])]
        only_unfused = sorted(n for n, w in rec["written"].items() if w and not d["written"][n])
        only_fused = sorted(n for n, w in d["written"].items() if w and not rec["written"][n])
        line = f"plan-arm inference {rec['case']}: written only without the chain kernel {only_unfused}, only with it {only_fused}"
        print(line)
        report(line)
        assert rec["written"][INFER_WITNESS] and not d["written"][INFER_WITNESS], rec["case"]
        for a, b in zip(rec["outputs"], d["outputs"]):
            assert torch.isfinite(a).all() and torch.equal(a, b), rec["case"]
