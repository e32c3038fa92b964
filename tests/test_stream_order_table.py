"""CPU: the table of tests/stream_order.py held to the header and to being a check, before tests/test_gpu_stream_order.py leans on it.

Every `int lfi_*` function of include/lfi.h is classified in stream_order.CLASSES — asynchronous, conditionally blocking (with the condition),
synchronous or host-only — so the next call added to the ABI fails here until someone has decided what it may do to the calling thread; and
every function that is asynchronous, always or under a condition, is called inside the stalled window of at least one script.  And for every
script, on the oracle alone: what each snapshot must show differs in at least half of its colour bytes from everything it could be confused
with — the same render from the other inputs, parameters, per-view rows or focus map of the script, and what the other snapshots show —
otherwise a call that jumped its stream order could still pass."""
import os
import re

import pytest

import lfinterpolator_amd as L
import stream_order as so
from conftest import ROOT


def _declared():
    with open(os.path.join(ROOT, "include", "lfi.h")) as f:
        text = f.read()
    return re.findall(r"^int\s+(lfi_\w+)\(", text, flags=re.M), re.findall(r"^const char \*\s*(lfi_\w+)\(", text, flags=re.M)


def _unclassified(declared, classes):
    return sorted(set(declared) - set(classes))


def test_every_function_of_the_header_is_classified():
    ints, strings = _declared()
    assert len(ints) > 80 and "lfi_render" in ints and "lfi_debug_streams" in ints and "lfi_last_error" in strings, "the header is no longer parsed"
    assert not _unclassified(ints + ["lfi_last_error", "lfi_last_kernel_name", "lfi_list_variants"], so.CLASSES), "declared in include/lfi.h, not classified in tests/stream_order.py"
    assert not sorted(set(so.CLASSES) - set(ints) - set(strings)), "classified but not declared"
    kinds = (so.ASYNC, so.COND, so.SYNC, so.HOST)
    assert all(kind in kinds for kind, _ in so.CLASSES.values())
    assert all(len(note) > 20 for kind, note in so.CLASSES.values() if kind == so.COND), "a conditionally blocking call names its condition"
    # the check itself: a function taken out of the classification is missed
    for name in ("lfi_render", "lfi_upload_mosaic_yuv_derived", "lfi_debug_streams"):
        fewer = {k: v for k, v in so.CLASSES.items() if k != name}
        assert _unclassified(ints, fewer) == [name]


def test_every_asynchronous_function_is_called_inside_a_stalled_window(oracle_c, native):
    used = set()
    for script in so.SCRIPTS:
        used |= so.dry_cached(L, oracle_c, script).used
    assert not sorted(used - set(so.CLASSES))
    must = {name for name, (kind, _) in so.CLASSES.items() if kind in so.MUST_BE_SCRIPTED}
    assert len(must) >= 20
    assert not sorted(must - used), "asynchronous by the header, in no script of tests/stream_order.py"
    # a step that may wait is marked and quotes why; the not-drained check is placed before the first of them
    for script in so.SCRIPTS:
        r = so.dry_cached(L, oracle_c, script)
        assert r.snapshots and len({label for label, _ in r.snapshots}) == len(r.snapshots), script.name


@pytest.mark.parametrize("script", so.SCRIPTS, ids=lambda s: s.name)
def test_no_snapshot_could_pass_for_another_state(script, oracle_c, native):
    worst, pairs = so.distinguishability(L, oracle_c, script)
    print(f"{script.name}: {pairs} pairs, the closest differ in {worst:.3f} of their colour bytes")
    assert pairs >= len(so.dry_cached(L, oracle_c, script).snapshots) and worst >= 0.5
