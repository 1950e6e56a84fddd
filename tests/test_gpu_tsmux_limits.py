"""GPU: the TS multiplexer and its remux (csrc/tsmux_kernels.hip, the remux part of csrc/stream_capi.cpp) at the widths
tests/tsmux_limit_cases.py takes them to -- eight live inputs, 64 map entries beside 64 tracked PIDs, calls past the
emit and the classify kernel's grids, a seeded sweep -- against the sequential references: bytes, both counter sets and
both resume positions, all exact.  Every run goes through the poisoned-buffer device_run of test_gpu_tsmux.py or
test_gpu_tsremux.py, which check the guards; tests/test_cpu_tsmux_limits.py shows what each case exercises."""
import numpy as np
import pytest

import dvbt2ll
from dvbt2ll.tsmux import TsRemuxPos
import test_gpu_tsmux as P
import test_gpu_tsremux as X
import tsmux_limit_cases as L
import tsremux_ref as XR

pytestmark = pytest.mark.gpu

SWEEP = L.sweep()


def _run(mux, case, n_out, start, rstart=None, align=(0, 0)):
    if case["remux"] is None:
        return P.device_run(mux, case["inputs"], n_out, start=start, align=align)
    return X.device_run(mux, case["inputs"], n_out, start, TsRemuxPos(*rstart), align=align)


def _same(res, case, ctx):
    ref, rref = L.reference(case)
    if rref is None:
        P.same(res, ref, ctx)
    else:
        X.same(res, ref, rref, ctx)


def _handle(case, max_out=None):
    if case["remux"] is None:
        return dvbt2ll.TsMux(max_out_packets=max_out or max(case["n_out"], 1), **case["mux"])
    return X.handle(case, max_out)


def _chained(mux, case, cuts, ctx, align=(0, 0)):
    """the call in pieces that end at cuts, each from the one before's resume positions: the single call's bytes, its
    resume positions, its counters summed"""
    ref, rref = L.reference(case)
    remux = rref is not None
    parts, pos, rpos = [], case["start"], case["rstart"] if remux else None
    for a, b in zip((0,) + tuple(cuts), tuple(cuts) + (case["n_out"],)):
        parts.append(_run(mux, case, b - a, pos, rpos, align=align))
        pos, rpos = parts[-1].resume, tuple(parts[-1].remux.resume) if remux else None
        align = align[::-1]
    np.testing.assert_array_equal(np.concatenate([p.ts for p in parts]), ref.ts, err_msg=str(ctx))
    assert tuple(pos) == tuple(ref.resume), (ctx, pos, ref.resume)
    assert X._sum([p.counters for p in parts]) == ref.counters, ctx
    if remux:
        assert rpos == tuple(rref.resume), (ctx, rpos, rref.resume)
        assert X._sum([p.remux.counters for p in parts]) == rref.counters, ctx


# ---------------------------------------------------------------------------------------- eight inputs
EIGHT = {"plain8": L.plain8(), "remux8": L.remux8()}


@pytest.fixture(scope="module", params=list(EIGHT))
def eight(request, gpu):
    """the case and one handle for all of its runs"""
    case = EIGHT[request.param]
    return case, _handle(case)


def test_eight_inputs_equal_the_reference(eight):
    """every staging lane, every restamp bit, every row of the PID map and every per-input result word is live: seven
    inputs are consumed, the eighth is a null pointer; remux8's start counters differ from nibble to nibble and from
    word to word"""
    case, mux = eight
    _same(_run(mux, case, 300, case["start"], case["rstart"], align=(3, 1)), case, case["name"])


def test_eight_inputs_every_output_alignment_against_every_input_alignment(eight):
    """input i lies at the first input's alignment + i, so each call has every relative alignment"""
    case, mux = eight
    for ao in range(4):
        for ai in range(4):
            _same(_run(mux, case, 300, case["start"], case["rstart"], align=(ao, ai)), case, (ao, ai))


def test_eight_inputs_splits_chain_to_the_single_call(eight):
    """k and 300 - k slots for every k up to two tiles and a bit, both positions carried"""
    case, mux = eight
    for k in range(138):
        _chained(mux, case, (k,), k, align=(k % 4, (k // 4) % 4))


def test_eight_inputs_run_host(eight):
    case, mux = eight
    if case["remux"] is None:
        P.same(mux.run_host(case["inputs"], 300, start=case["start"]), L.reference(case)[0], "host")
    else:
        _same(mux.run_host_remux(case["inputs"], 300, start=case["start"], rstart=TsRemuxPos(*case["rstart"])), case, "host")


def test_an_empty_remux_gives_the_plain_handles_bytes_at_eight_inputs(gpu):
    case = EIGHT["plain8"]
    ref, _ = L.reference(case)
    mux = dvbt2ll.TsMux(max_out_packets=300, **case["mux"])
    mux.set_remux()
    got = X.device_run(mux, case["inputs"], 300, case["start"], TsRemuxPos(), align=(2, 3))
    plain = P.device_run(P.mux_of(**case["mux"])[0], case["inputs"], 300, start=case["start"], align=(1, 0))
    np.testing.assert_array_equal(got.ts, plain.ts)
    P.same(got, ref, "empty remux")
    assert got.remux.counters == dict.fromkeys(XR.REMUX_COUNTERS, 0) and got.remux.resume == TsRemuxPos()


# ---------------------------------------------------------------------------------------- past the grids
def test_long_emit_past_the_emit_grid(gpu):
    """the emit kernel's second trip, where rec, the ballot rank and the LDS counters are used again, with a short last
    tile, and a second scan round over nine chunks; then the call cut at the trip's and at the chunk's first packet"""
    case = L.long_emit()
    ref, rref = L.reference(case)
    assert rref.counters["cc_rewritten"] > 100000 and rref.counters["pcr_restamped"] > 1000 and rref.counters["remapped"] > 1000
    mux = _handle(case)
    _same(_run(mux, case, case["n_out"], case["start"], case["rstart"], align=(1, 2)), case, "whole")
    _chained(mux, case, (L.MAX_BLOCKS * L.TILE,), "cut at the second trip", align=(2, 0))
    _chained(mux, case, (L.TILE * L.SCAN_TILES,), "cut at the second chunk", align=(0, 3))


def test_long_classify_past_the_classify_grid(gpu):
    """the classify kernel's second trip, where the four LDS rows are used again, the emit kernel's fifth, and a second
    scan round over 33 chunks: one run into one output"""
    case = L.long_classify()
    ref, rref = L.reference(case)
    assert rref.counters["cc_rewritten"] == 494705 and len(ref.ts) == 524359 * 188
    _same(_run(_handle(case), case, case["n_out"], case["start"], case["rstart"], align=(3, 0)), case, "whole")


# ---------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("k", range(len(SWEEP)), ids=[c["name"] for c in SWEEP])
def test_sweep_case_equals_the_reference_whole_and_split(gpu, k):
    case = SWEEP[k]
    mux = _handle(case)        # a remux handle cannot be shared: set_remux comes before its first run
    _same(_run(mux, case, case["n_out"], case["start"], case["rstart"], align=(k % 4, (k // 4) % 4)), case, case["name"])
    _chained(mux, case, (case["split"],), (case["name"], case["split"]), align=((k + 1) % 4, (k // 4 + 2) % 4))
