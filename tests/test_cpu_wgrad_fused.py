import os

from pointcloudprocessing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wgrad_fused_entries():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "pointnet_hip.h")).read()
    for name in ("pn_conv_bwd_data_wgrad", "pn_model_wgrad_fused_count"):
        assert hasattr(L, name) and name in hdr, name
    assert int(L.pn_model_wgrad_fused_count()) >= 0            # GEMMs planned fused since the library was loaded
    assert "#define PN_ABI_VERSION 6" in hdr and int(L.pn_model_plan_count(3)) == -1
