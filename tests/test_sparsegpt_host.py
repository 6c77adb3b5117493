"""CPU: the host decisions of vlmc/sparsegpt.py that need no device.

`_pick_attempt` is what `factorize_many` does with the flags of one input's damping attempts after its one host read.  A
flag pair is [not clean, NaN in the inverse factor without a failed pivot] (the second implies the first); the pairs come in
k order.  The expected outcomes are the rules `factorize_many` had written out once per round before the two rounds shared
this function:
  round one -- no clean attempt: the reference chain if ANY attempt is NaN-only, else a retry with the next two k; a clean
               attempt: the reference chain if an attempt BEFORE it is NaN-only, else that attempt;
  round two -- a clean attempt with no NaN-only attempt before it is taken; everything else goes to the reference chain."""
import pytest

CLEAN, FAILED, NAN_ONLY = [False, False], [True, False], [True, True]

TABLE = [
    # flags in k order, after round one, after round two
    ([CLEAN], ("take", 0), ("take", 0)),                                 # an input with a clean history: k = 0 alone
    ([CLEAN, CLEAN], ("take", 0), ("take", 0)),                          # clean at k = 0: the damped attempt is not looked at
    ([CLEAN, FAILED], ("take", 0), ("take", 0)),
    ([FAILED, CLEAN], ("take", 1), ("take", 1)),                         # clean at k = 1 (a singular H)
    ([NAN_ONLY, CLEAN], ("reference",), ("reference",)),                 # an EARLIER attempt factorized but left NaN
    ([CLEAN, NAN_ONLY], ("take", 0), ("take", 0)),                       # a NaN-only attempt AFTER the first clean one: ignored
    ([FAILED], ("retry",), ("reference",)),                              # all bad: the next two k, then the reference's loops
    ([FAILED, FAILED], ("retry",), ("reference",)),
    ([FAILED, NAN_ONLY], ("reference",), ("reference",)),                # none clean and one NaN-only: not a case for more damping
    ([NAN_ONLY, FAILED], ("reference",), ("reference",)),
]


@pytest.mark.parametrize("flags,first,second", TABLE)
def test_pick_attempt_decides_like_both_rounds_of_factorize_many_did(flags, first, second):
    from vlmc.sparsegpt import _pick_attempt
    assert _pick_attempt(flags) == first
    assert _pick_attempt(flags, last_round=True) == second
