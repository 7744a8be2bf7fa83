"""CPU suite of the capture-and-replay table (tests/util_graph_replay.py): the table imports without a GPU and its inputs are two
different problems per case; the stream-taking entries parsed from include/pdepth.h are exactly those of the binding's signature
table, so that a new entry cannot be added without a row; every float-atomics rule names a callable of an existing suite."""
import ctypes

import pytest
import torch

import pdepth_amd  # noqa: F401
from pdepth_amd import _native
import util_graph_replay as G


def test_stream_entries_of_the_header_are_those_of_the_signature_table():
    """In _native._SIGNATURES an entry that launches returns a status (c_int) and takes the stream, a void pointer, last; the
    queries return a size, a layout or a string, or fill integers.  The header's prototypes with `void *stream` must be exactly
    those: a new entry then cannot be added without a row in the table (tests/test_graph_replay_gpu.py holds the union of the
    rows to this set)."""
    from_header = G.stream_entries()
    launching = {n for n, (restype, argtypes) in _native._SIGNATURES.items()
                 if restype is ctypes.c_int and argtypes and argtypes[-1] is ctypes.c_void_p}
    assert len(from_header) == len(set(from_header))
    assert set(from_header) == launching, sorted(set(from_header) ^ launching)
    assert len(from_header) == 63, len(from_header)
    print("%d entries take a stream, %d are host-side queries" % (len(from_header), len(_native._SIGNATURES) - len(from_header)))


def _differs(a, b):
    keys = [k for k, v in a.items() if isinstance(v, torch.Tensor)]
    assert keys and set(a) == set(b)
    return [k for k in keys if a[k].shape == b[k].shape and not torch.equal(a[k], b[k])], keys


@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_IDS)
def test_inputs_of_the_two_seeds_differ(case):
    a, b = case.make_inputs(0), case.make_inputs(1)
    changed, keys = _differs(a, b)
    scaled = a.get("_scaled", ())
    assert set(scaled) <= set(keys), scaled
    assert all(a[k].numel() <= G.MAX_ELEMENTS for k in keys)
    assert all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in keys)   # B goes into A's captured buffers
    # every tensor B scales differs already by its seed, and so does something that decides where a scatter lands or what is read
    assert set(scaled) <= set(changed) and len(changed) > len(scaled), (changed, scaled)
    again, _ = _differs(a, case.make_inputs(0))
    assert not again, again   # the same seed gives the same tensors
    sb = G.scaled(b)
    assert all(torch.equal(sb[k], b[k] * 2.0 ** 5) for k in scaled)


def test_every_atomic_rule_names_a_callable_of_an_existing_suite():
    rules = G.atomic_rules()
    assert {c for c, _, _ in rules} == {c.name for c in G.CASES if c.name.endswith("-atomic")}
    for case, output, rule in rules:
        fn = rule.resolve()
        print(case, output, rule.source)
        assert callable(fn) and not rule.source.startswith("util_graph_replay"), (case, rule.source)
        assert callable(rule.det_step) and callable(rule.reference) and callable(rule.check)
    # each scattered gradient of the ABI has both of its paths in the table
    names = set(G.CASE_IDS)
    assert all(n[:-len("atomic")] + "det" in names for n in names if n.endswith("-atomic"))


def test_recorder_notes_entries_and_passes_everything_else_through():
    class Lib:
        other = 7

        def pdepth_abi_version(self):
            return 6

    seen = set()
    proxy = G.Recorder(Lib(), seen)
    assert proxy.other == 7 and not seen
    assert proxy.pdepth_abi_version() == 6 and seen == {"pdepth_abi_version"}
    assert getattr(proxy, "pdepth_missing", None) is None and not hasattr(proxy, "pdepth_missing")
