"""CPU model check of the greedy decode's exit protocol (tests/greedy_exit_model.py): over every interleaving of two batch tiles'
reduced chains, no deadlock, every token below n_steps written, no workgroup leaving below n_steps, n_steps = the first step at which
every row is done, and the finishing tile stopping at n_steps; and the checker flags the two mutations."""
import pytest

from greedy_exit_model import explore

CASES = [
    [[0, 0], [0, 0]],          # every row at EOS on step 0: n_steps = 1
    [[2], [1]],                # the tiles finish at different steps
    [[0, 2], [1, 1]],          # rows of one tile at different steps
    [[1, 2], [None, 0]],       # one row never: n_steps = stop_limit
    [[None], [None]],          # no EOS at all
    [[3], [3]],                # on the last step
]


@pytest.mark.parametrize("eos", CASES)
def test_protocol_holds_over_every_interleaving(eos):
    violations, n_states = explore(eos, stop_limit=4)
    assert not violations, violations
    assert n_states > 100


@pytest.mark.parametrize("eos", [[[0, 0], [0, 0]], [[2], [1]]])
def test_stop_word_after_the_ce_arrival_is_flagged(eos):
    violations, _ = explore(eos, stop_limit=4, late_stop=True)
    assert "overrun" in violations, violations


@pytest.mark.parametrize("role", ["att", "ctx", "log", "ce"])
def test_a_wait_without_the_stop_check_is_flagged(role):
    violations, _ = explore([[2], [1]], stop_limit=4, no_check=role)
    assert "deadlock" in violations, violations


def test_cells_without_the_stop_check_are_flagged():
    """Cells that never read the stop word run the finishing tile past n_steps."""
    violations, _ = explore([[2], [1]], stop_limit=4, no_check="cell")
    assert "overrun" in violations, violations
