"""Host side of the pnr_aggregate_fwd*_p1 entry points (ABI 33, no GPU): P1 in a table of the caller's.
What tests/test_aggregate_host.py checks for the three calls they extend, plus the table's own refusals
and the smaller scratch; every accepted call has n_max = 0 and returns before any HIP call."""
import ctypes

import pytest

from test_aggregate_host import FAKE, ODD, Call, L, _ref, _set  # noqa: F401  (L: the module's fixture)

P1 = {"pnr_aggregate_fwd_p1": "pnr_aggregate_fwd", "pnr_aggregate_fwd_x3_p1": "pnr_aggregate_fwd_x3",
      "pnr_aggregate_fwd_h2_p1": "pnr_aggregate_fwd_h2"}


def _run(L, name, change=None, table=FAKE):
    c = Call(L, P1[name])
    nb = ctypes.c_size_t(0)
    assert L.lib().pnr_aggregate_scratch_bytes(0, 0, ctypes.byref(nb)) == L.PNR_OK
    assert 0 < nb.value < c.scratch_bytes      # no P1 rows in the scratch
    c.scratch_bytes = nb.value
    if change is not None:
        change(c)
    args = c.args()
    k = len(args) - 6                          # behind the packs, in front of out_feat
    return getattr(L.lib(), name)(*args[:k], table, *args[k:])


@pytest.mark.parametrize("name", P1)
def test_p1_call_without_samples_returns_ok_on_the_small_scratch(L, name):
    assert _run(L, name) == L.PNR_OK


@pytest.mark.parametrize("name", P1)
def test_p1_call_refusals(L, name):
    assert _run(L, name, table=None) == L.PNR_EINVAL and b"null p1_table" in L.lib().pnr_last_error()
    assert _run(L, name, table=ODD) == L.PNR_EINVAL and b"p1_table must be 16-B aligned" in L.lib().pnr_last_error()

    def short(c):
        c.scratch_bytes -= 1
    assert _run(L, name, short) == L.PNR_EINVAL and b"scratch too small" in L.lib().pnr_last_error()
    assert _run(L, name, _set("pts", "emb", None)) == L.PNR_EINVAL and b"xyz/emb required" in L.lib().pnr_last_error()


def test_plain_calls_still_need_the_p1_rows_in_the_scratch(L):
    for name in P1.values():
        c = Call(L, name)
        nb = ctypes.c_size_t(0)
        L.lib().pnr_aggregate_scratch_bytes(0, 0, ctypes.byref(nb))
        c.scratch_bytes = nb.value
        assert c.run() == L.PNR_EINVAL and b"scratch too small" in L.lib().pnr_last_error()
