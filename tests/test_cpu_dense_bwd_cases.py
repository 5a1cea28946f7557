"""The dense-backward cases of tests/test_gpu_ops.py are compared with fp64 autograd, whose answer is arbitrary for an element on the
ReLU boundary.  No GPU is needed to know whether a case has such an element: the GPU is handed float(z_ref), so the decision is made
on the values replayed here.  A case that had one used to skip on every run; now its seed is chosen so that it has none."""
import pytest

from test_gpu_ops import DENSE_BWD_CASES, DENSE_BWD_SEED_K, dense_bwd_case


@pytest.mark.parametrize("R,K,C_,bn_mode,act,drop", DENSE_BWD_CASES)
def test_no_dense_bwd_case_has_an_element_on_the_relu_boundary(R, K, C_, bn_mode, act, drop):
    assert dense_bwd_case(R, K, C_, bn_mode, act, drop)["on_boundary"] == 0


def test_seed_table_names_only_listed_cases():
    assert set(DENSE_BWD_SEED_K) <= set(DENSE_BWD_CASES)
