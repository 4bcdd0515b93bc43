"""The corner images of tests/history_edge_grid_cases.py on a real MI355X: the
fold, joint, corr, period, shift and match kernels of
src/gpu/kernels/history.hip against the NumPy references (images 1 to 9 and
the cell images: each query's own assert_same, a second run's bytes, the host
twin as the query's own GPU test compares it) and against the invariants of a
ring out of time order (image 10).  tests/test_history_edge_grid_cpu.py shows
that each image reaches the path it is for."""
import pytest

import history_edge_cases as E
import history_edge_grid_cases as EG

pytestmark = pytest.mark.gpu
BY_ID = dict(ids=lambda c: c[0])
BY_LABEL = dict(ids=lambda g: g["label"])


@pytest.fixture(scope="module")
def lib(native_built):
    return native_built.load_gpu_lib()


@pytest.mark.parametrize("case", EG.windows(), **BY_ID)
def test_fold_matches_reference(lib, case):
    EG.check_fold(lib, case, use_host=0, twin=True)


@pytest.mark.parametrize("case", EG.windows(), **BY_ID)
def test_joint_matches_reference(lib, case):
    EG.check_joint(lib, case, use_host=0, twin=True)


@pytest.mark.parametrize("case", EG.windows(), **BY_ID)
def test_corr_matches_reference(lib, case):
    EG.check_corr(lib, case, use_host=0, twin=True)


@pytest.mark.parametrize("g", EG.grids(), **BY_LABEL)
def test_period_matches_reference(lib, g):
    EG.check_period(lib, g, use_host=0, twin=True)


@pytest.mark.parametrize("g", EG.grids(), **BY_LABEL)
def test_shifts_match_reference(lib, g):
    EG.check_shifts(lib, g, use_host=0, twin=True)


@pytest.mark.parametrize("g", EG.match_grids(), **BY_LABEL)
def test_match_matches_reference(lib, g):
    EG.check_match(lib, g, use_host=0, twin=True)


@pytest.mark.parametrize("case", E.out_of_order_cases(), **BY_ID)
def test_out_of_order_invariants(lib, case):
    EG.check_out_of_order(lib, case, use_host=0)
