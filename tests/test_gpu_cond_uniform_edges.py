"""
The look-aheads of cond_uniform_kernel (the record-free condensing of a stage-uniform iterate, POWER form, options_set("uniform_powers", 1))
at the horizons where one can go wrong. The five-tile build requests what a stage's matrix instructions take -- the B operands of the
Hessian tiles, the weight of the lane's operand row, the gg-row entries -- one stage ahead, into a second register set; the residual lanes
hold the reference two stages ahead. Each of them has an end (the last stage requests nothing) and the operand set changes shape on the
way: the first stage of a segment of eight has one tile more than the stage that requests its operands, and stage 33 is the first with
the columns beyond 64 (bank 1).

Every case is a pair of TWIN capsules built exactly as tests/test_gpu_uniform_powers.py builds them (weights different at every stage and
instance, yaws on both sides of +-pi, batch 1025: the smallest that takes the record-free chain) that differ in "uniform_powers" only:
1, the kernel under test, against 0, the column form (cond_uniform_columns_kernel), which has no look-ahead of this kind and is untouched.

Bound: bit equality (np.array_equal) of X, U, cost, status, qp_iter, qp_status, res, sl, su and lam -- the look-ahead moves reads, not
arithmetic: every sum takes the same operands in the same order. Both twins must report records_skipped == 1, and a second solve on the
now non-uniform iterate (cond_kernel on both) must agree as well.

Horizons (all accepted by the library: 1 is its smallest):
  1, 2, 3     the guards at the end: the reference two stages ahead and the request one stage ahead stop before the horizon does.
              (At 1025 instances the library linearises horizons up to 6 with eight lanes per stage, which keeps the records: the twins
              of these three are told set_kernel("lin-lane-per-stage"), the choice of every larger batch, and then take the record-free
              chain at batch 1025 like the others -- records_skipped says so.)
  8, 16       the last stage closes a segment (nothing behind it: no request with one tile more)
  9, 17, 25   the last stage is the first of a segment: its operands were requested by the stage that closes the segment before
  33          bank 1's first stage is the last stage: its gg-row entry and operands were requested by stage 32
and the reset case of tests/test_gpu_uniform_records.py (X = 0, U = 0: the linearisation fails and leaves NaN) at N = 9.
"""
import pytest

from test_gpu_uniform_powers import B0, _assert_same, _mk, _snap

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [1, 2, 3, 8, 16, 9, 17, 25, 33])
def test_look_ahead_at_the_edges_equals_column_form(N):
    p, c = _mk(N, 1), _mk(N, 0)
    for s in (p, c):
        if 1025 * (N + 1) * 8 <= 64 * 1024:
            s.set_kernel("lin-lane-per-stage")
        s.cold_start()
        s.solve()
    assert p.get_stats("records_skipped") == 1 and c.get_stats("records_skipped") == 1
    a, b = _snap(p), _snap(c)
    print(f"N={N}: instances solved", int((a["status"] == 0).sum()), "of", B0, "qp_iter", int(a["qp_iter"].min()), "..", int(a["qp_iter"].max()))
    _assert_same(a, b, f"N={N}")
    # the second solve: the iterate is uniform no more, cond_kernel runs on both
    for s in (p, c):
        s.solve()
    assert p.get_stats("records_skipped") == 1 and c.get_stats("records_skipped") == 1
    _assert_same(_snap(p), _snap(c), f"N={N}, second solve")
    p.synchronize(); c.synchronize()


def test_reset_equals_column_form_where_a_segment_opens():
    """reset(): X = 0, U = 0 at every stage -- the vehicle at rest, the linearisation carries NaN; N = 9: the last stage opens a segment"""
    p, c = _mk(9, 1), _mk(9, 0)
    for s in (p, c):
        s.cold_start(); s.solve()
        s.reset(); s.solve()
    assert p.get_stats("records_skipped") == 2 and c.get_stats("records_skipped") == 2
    _assert_same(_snap(p), _snap(c), "after reset()")
    p.synchronize(); c.synchronize()
