"""Keeps the table of environment switches honest without a GPU: every PN_* name the library or engine.py reads from the environment has
exactly one home -- an arm of tests/test_gpu_plan_arms.py, another test that flips it, or the list of ablations whose results are wrong
or unchanged by design.  A new switch without a home fails here.  Next to it, what wgrad_slab_rows (pn_model.hip) returns at the
values the slab-count arms use, restated on the CPU: the arms rely on these."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointcloudprocessing_amd", "csrc")

# flipped by another test: name -> the file that does it
FLIPPED_ELSEWHERE = {
    "PN_SLAB_DEFER": "test_gpu_train.py",
    "PN_WGRAD_BATCH": "test_gpu_train.py",
    "PN_GW_BATCH": "test_gpu_train.py",
    "PN_DDP_OVERLAP": "test_gpu_train.py",
    "PN_WGRAD_FUSE": "test_gpu_wgrad_fused.py",
    "PN_PREP_CARRY": "test_gpu_carry.py",
    "PN_DR64_RIDE": "test_gpu_carry.py",
    "PN_FPS_PRUNE": "test_gpu_fps.py",
    "PN_KNN_SPLIT": "test_gpu_scan_propagation.py",
    "PN_WS_GUARD": "test_gpu_model.py",
}
# ablations: a probe switches a part of a kernel OFF or makes it write time stamps, so the results are wrong (or, for the stamps,
# unchanged) by design and no parity test can hold them to anything
ABLATIONS = {
    "PN_GEMM_DBG": "row-GEMM probe: skips the staging / the MFMAs / the epilogue of a tile",
    "PN_PANEL_DBG": "panel-kernel probe: skips phases of the kernel, 16 writes time stamps (tools/panel_probe.py, tools/panel_stamps.py)",
    "PN_SCATTER_DBG": "max-pool backward scatter probe: skips the row lookup / the scatter / the store",
    "PN_SEGHEAD_DBG": "fused segmentation head: 16 writes time stamps into the partial-sum buffer (tools/seghead_stamps.py)",
}


def plan_arm_switches():
    import test_gpu_plan_arms as T
    names = set(T.SEGHEAD_ARM) | set(T.INFER_ARM)
    for env, _ in T.TRAIN_ARMS.values():
        names |= set(env)
    return names


def switches_read():
    files = glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(ROOT, "pointcloudprocessing_amd", "engine.py")]
    assert len(files) > 20
    pat = re.compile(r"(?:getenv|env_on|env_int|environ\.get)\(\s*\"(PN_[A-Z0-9_]+)\"")
    found = {}
    for f in files:
        with open(f) as fh:
            for name in pat.findall(fh.read()):
                found.setdefault(name, os.path.basename(f))
    return found


def test_every_environment_switch_has_exactly_one_home():
    found = switches_read()
    arms = plan_arm_switches()
    # the scan itself works: one name from each reader
    assert {"PN_PM_IN_PREP", "PN_DENSE_KSPLIT", "PN_SEGHEAD_MB", "PN_DDP_OVERLAP", "PN_WS_GUARD"} <= set(found)
    homes = {n: [h for h, s in (("plan arm", arms), ("flipped elsewhere", FLIPPED_ELSEWHERE), ("ablation", ABLATIONS)) if n in s] for n in found}
    assert {n: h for n, h in homes.items() if len(h) != 1} == {}, "a switch needs exactly one home (a plan arm, another test, or the ablation list)"
    stale = (arms | set(FLIPPED_ELSEWHERE) | set(ABLATIONS)) - set(found)
    assert stale == set(), f"listed but read nowhere: {sorted(stale)}"
    for name, fname in FLIPPED_ELSEWHERE.items():
        with open(os.path.join(ROOT, "tests", fname)) as fh:
            assert name in fh.read(), f"{fname} does not mention {name}"
    assert all(len(reason) > 10 for reason in ABLATIONS.values())


def test_pm_small_is_compared_under_its_own_launch():
    """PN_PM_SMALL acts only where the Pm launch exists (PN_PM_IN_PREP=0): the digest test must take both digests there"""
    with open(os.path.join(ROOT, "tests", "test_gpu_train.py")) as fh:
        src = fh.read()
    assert "digest(PN_PM_IN_PREP=0, PN_PM_SMALL=0)" in src and "digest(PN_PM_IN_PREP=0)" in src


def cdiv(a, b):
    return -(-a // b)


def wgrad_slab_rows(B, N, Ci, Cj, target):
    """pn_model.hip: wgrad_slab_rows, restated: (rows per slab, slabs per cloud)"""
    bm = 128 if (Ci % 128 == 0 and Cj % 128 == 0) else 64
    bn = 128 if Cj % 128 == 0 else 64
    target = max(1, target // ((Ci // bm) * (Cj // bn)))
    spc = max(1, min(cdiv(target, B), cdiv(N, 64)))
    rows = cdiv(cdiv(N, spc), 64) * 64
    return rows, cdiv(N, rows)


JOBS = [(64, 64), (64, 128), (128, 128), (64, 512), (512, 256), (256, 128)]


def test_the_slab_count_arms_reach_long_slabs():
    """the restated function is the C++ one line for line (checked against the source's distinctive lines), and at the arms' values it
    gives what tests/test_gpu_plan_arms.py states: PN_WGRAD_TARGET=8 a slab of more than 64 rows for some job at every case (at B = 5,
    N = 200 the two-tile slab with a ragged second slab of 72 rows), PN_WGRAD_TARGET=1 one slab per cloud for every job"""
    with open(os.path.join(CSRC, "pn_model.hip")) as fh:
        src = fh.read()
    for line in ("int target = (target_override > 0 ? target_override : sw().wgrad_target) / n_out;", "int spc = cdiv(target, B);",
                 "const int max_spc = cdiv(N, 64);", "int rows = cdiv(cdiv(N, spc), 64) * 64;", "spc = cdiv(N, rows);"):
        assert line in src, line
    # the default plan at the small parity shapes sits at the 64-row floor
    assert all(wgrad_slab_rows(5, 200, ci, cj, 256) == (64, 4) for ci, cj in JOBS)
    assert all(wgrad_slab_rows(4, 384, ci, cj, 256) == (64, 6) for ci, cj in JOBS)
    assert [wgrad_slab_rows(40, 136, ci, cj, 256) for ci, cj in JOBS] == [(64, 3), (64, 3), (64, 3), (128, 2), (192, 1), (64, 3)]
    # few slabs
    assert [wgrad_slab_rows(5, 200, ci, cj, 8) for ci, cj in JOBS] == [(128, 2)] * 3 + [(256, 1)] * 3
    assert 200 - 128 == 72
    assert all(wgrad_slab_rows(40, 136, ci, cj, 8) == (192, 1) for ci, cj in JOBS)
    # two long ragged clouds (tests/test_gpu_plan_arms.py: LONG_RAGGED): 64-row slabs by default, 576 rows with a ragged last slab at 8
    assert [wgrad_slab_rows(2, 2100, ci, cj, 256) for ci, cj in JOBS] == [(64, 33), (64, 33), (64, 33), (128, 17), (192, 11), (64, 33)]
    assert [wgrad_slab_rows(2, 2100, ci, cj, 8) for ci, cj in JOBS] == [(576, 4)] * 3 + [(2112, 1), (2112, 1), (1088, 2)]
    assert 2100 - 3 * 576 == 372 == 5 * 64 + 52 and 2100 - 1088 == 1012
    # one slab per cloud
    assert all(wgrad_slab_rows(5, 200, ci, cj, 1) == (256, 1) for ci, cj in JOBS)
    # the Pm job of PN_PM_IN_PREP=0: B = 1, the 1024 channels as rows
    assert [wgrad_slab_rows(1, 1024, 128, 128, t) for t in (256, 8, 1)] == [(64, 16), (128, 8), (1024, 1)]
