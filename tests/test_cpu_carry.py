"""host side of the carried launches' introspection entry (the GPU side: tests/test_gpu_carry.py)"""
from pointcloudprocessing_amd import _lib


def test_plan_count_entry():
    L = _lib.lib()
    assert all(int(L.pn_model_plan_count(i)) >= 0 for i in range(3))           # counts since the library was loaded
    assert int(L.pn_model_plan_count(3)) == -1 and int(L.pn_model_plan_count(-1)) == -1
