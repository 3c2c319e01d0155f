"""A handle gives back everything it took: the device memory that is free after four whole lives of a handle (tests/handle_cycles.py) is
still free after twelve, the lives of the two handles that fail on the way included.  Measured as
test_workspace_bytes_bounds_what_a_forward_reserves measures: free HBM from torch.cuda.mem_get_info, corrected by
torch.cuda.memory_reserved.  The bound is the drift of the same cycles on the commit before the handle owned its members by type,
which was 0 bytes on both handles (profiles/forward_units_refactor.md)."""
import pytest

from tests import handle_cycles

pytestmark = pytest.mark.gpu

ALLOWED_GROWTH = 0          # bytes over cycles 5..12: what the parent commit drifted by


@pytest.mark.parametrize("name", sorted(handle_cycles.HANDLES))
def test_twelve_lives_of_a_handle_leave_free_memory_where_four_left_it(name):
    after = handle_cycles.cycles(name, 12)
    print(name, "free bytes after each cycle, relative to cycle 4:", [a - after[3] for a in after])
    assert after[3] - after[11] <= ALLOWED_GROWTH, (after[3], after[11])
