"""The corner images of tests/history_edge_cases.py on a real MI355X: the
kernels of src/gpu/kernels/history.hip, all four queries, against the NumPy
references (images 1 to 9: integer fields and bit patterns exactly, the fp64
sums within the summation bound, a second run's bytes, the host twin's exact
fields) and against the invariants of a ring out of time order (image 10).
tests/test_history_edge_cases_cpu.py shows that each image reaches the path
it is for."""
import pytest

import history_edge_cases as E
from dynolog_amd.utils import slots as S

pytestmark = pytest.mark.gpu
BY_ID = dict(ids=lambda c: c[0])


@pytest.fixture(scope="module")
def lib(native_built):
    return native_built.load_gpu_lib()


@pytest.mark.parametrize("case", E.cases(), **BY_ID)
def test_plain_matches_reference(lib, case):
    E.check_plain(lib, case, use_host=0, twin=True)


@pytest.mark.parametrize("case", [c for c in E.cases() if c[7] <= S.HISTORY_QUANTILE_MAX_BUCKETS], **BY_ID)
def test_quantiles_match_reference(lib, case):
    E.check_quantiles(lib, case, use_host=0, twin=True)


@pytest.mark.parametrize("case", E.episode_cases(), **BY_ID)
def test_episodes_match_reference(lib, case):
    E.check_episodes(lib, case, use_host=0, twin=True)


@pytest.mark.parametrize("case", E.cases(), **BY_ID)
def test_by_phase_matches_reference(lib, case):
    E.check_by_phase(lib, case, use_host=0, twin=True)


@pytest.mark.parametrize("case", E.out_of_order_cases(), **BY_ID)
def test_out_of_order_invariants(lib, case):
    E.check_out_of_order(lib, case, use_host=0)
