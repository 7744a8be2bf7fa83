"""GPU suite: every entry of include/pdepth.h that takes a stream, held to the header's promise (lines 13-14: asynchronous
launches, no host synchronisation, no allocation) by capture and replay -- tests/util_graph_replay.py has the protocol and the
table.  One parametrised test over the table; a test that the protocol can fail; and the coverage: the C entries the cases called,
noted by a proxy around what _native.load() returns, are all of the stream-taking entries but those that already have a capture
test of their own.  Everything asserted is printed."""
import importlib

import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native
import util_graph_replay as G

pytestmark = pytest.mark.gpu

# entry -> why no row of the table has to reach it.  Only entries with a capture test of their own, named "module::test" (the
# coverage test checks that it exists); nothing else is excluded: the header promises the contract of every entry.
EXCLUDED = {
    "pdepth_sweep_dpv_f32": "tests/test_round6_rows.py::test_nchw_entry_is_capturable",
    "pdepth_sweep_dpv_packed_f32": "tests/test_round4_rows.py::test_packed_entry_is_one_capturable_launch",
    "pdepth_lidar_depth_f32": "tests/test_lidar_gpu.py::test_call_is_capturable",
}
_called = {}   # case name -> the C entries its eager and captured runs called


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    return torch.device("cuda:0")


@pytest.fixture
def recorded():
    """The library behind _native.load() wrapped for the duration of a test: -> the set of entry names called."""
    real, seen = _native.load(), set()
    _native._lib = G.Recorder(real, seen)
    try:
        yield seen
    finally:
        _native._lib = real


@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_IDS)
def test_replays_equal_the_eager_step(dev, recorded, case):
    figures = G.check_replays(case.make_inputs, case.step, case.rules, tag=case.name)
    _called[case.name] = set(recorded)
    print("%s called %s" % (case.name, ", ".join(sorted(recorded))))
    atomic = [n for n, r in case.rules.items() if isinstance(r, G.Atomic)] if isinstance(case.rules, dict) else []
    assert len(figures) >= len(G.ORDER) * len(atomic)   # every replay of an atomic output was measured against its bound


def test_the_protocol_reports_a_stale_accumulator(dev):
    """A pure-torch step with a state: under capture acc.add_(x) goes into a persistent buffer that nothing clears, where the eager
    step starts from zero -- a clear that did not make it into the graph.  The first replay (acc = 0 + A) equals the eager step;
    the second (acc = A + B) does not, and the protocol says so.  No kernel of the library runs here."""
    acc = torch.zeros(2, 7, 9, device=dev)

    def make_inputs(seed):
        return {"x": torch.randn(2, 7, 9, generator=torch.Generator().manual_seed(seed)), "_scaled": ("x",)}

    def step(inp):
        if not torch.cuda.is_current_stream_capturing():
            return {"y": inp["x"] + 0.0}
        acc.add_(inp["x"])
        return {"y": acc + 0.0}

    lines = []
    with pytest.raises(AssertionError) as err:
        G.check_replays(make_inputs, step, G.BITS, log=lines.append, tag="stale accumulator")
    print(err.value)
    assert "replay 2 (B)" in str(err.value) and "output y" in str(err.value)
    # ... and a step without a state passes: the comparison is not what fails
    G.check_replays(make_inputs, lambda inp: {"y": inp["x"] * 3.0}, G.BITS, log=lines.append, tag="stateless")
    assert any("replays 1:A 2:B 3:A 4:A" in line for line in lines), lines


def test_the_protocol_reports_a_state_that_the_third_replay_meets(dev):
    """The other kind: a header word that keeps the largest magnitude ever seen (an exponent chosen per item and never reset).  A,
    then B = 2^5 times larger, are right; A after B meets B's word."""
    peak = torch.zeros((), device=dev)

    def make_inputs(seed):
        return {"x": torch.randn(64, generator=torch.Generator().manual_seed(seed)) + 3.0 * seed, "_scaled": ("x",)}

    def step(inp):
        top = inp["x"].abs().max()
        if torch.cuda.is_current_stream_capturing():
            peak.copy_(torch.maximum(peak, top))
            top = peak
        return {"y": torch.round(inp["x"] / top * 1024.0) / 1024.0 * top}

    with pytest.raises(AssertionError) as err:
        G.check_replays(make_inputs, step, G.BITS, log=lambda line: None, tag="stale exponent")
    print(err.value)
    assert "replay 3 (A)" in str(err.value)


def test_every_stream_entry_was_replayed():
    """The union of what the cases called holds every stream-taking entry of the header but EXCLUDED, whose entries name an
    existing capture test each."""
    assert len(_called) == len(G.CASES), "run the whole module: %d of %d cases ran" % (len(_called), len(G.CASES))
    want = set(G.stream_entries())
    assert want <= set(_native._SIGNATURES) and set(EXCLUDED) <= want
    for entry, reason in EXCLUDED.items():
        path, test = reason.split("::")
        module = importlib.import_module(path[len("tests/"):-len(".py")])
        assert callable(getattr(module, test)), reason
    further = [e for e, reason in EXCLUDED.items() if "::test_" not in reason]
    assert len(further) <= 3, further
    reached = set().union(*_called.values())
    missing = sorted(want - reached - set(EXCLUDED))
    print("%d stream-taking entries: %d replayed by the table, %d left to their own capture tests (%d of those replayed here as well)"
          % (len(want), len(want & reached), len(EXCLUDED), len(set(EXCLUDED) & reached)))
    for entry in sorted(want & reached):
        print("  %s: %s" % (entry, ", ".join(sorted(c for c, seen in _called.items() if entry in seen)[:4])))
    assert not missing, missing
