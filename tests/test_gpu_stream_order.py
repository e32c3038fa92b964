"""GPU: every script of tests/stream_order.py with one stream stalled — on the compute stream, on the copy stream, on the side stream.

Each case runs its script once un-stalled on a fresh context (every first-use allocation happens there, and the host time the script takes
to issue sizes the stall: five times that, between 50 and 500 ms), then again behind a finite spin on the chosen stream.  Three checks, all
from the host: the other streams' canary events complete while the stall is pending (or the case FAILS: streams that share a hardware queue
serialise behind the stall, and the run would prove nothing); the stall is still pending when the last call that lfi.h documents as
asynchronous has returned; and after the stall every snapshot of the attached views, the final focus maps and the comparison's numbers are
the oracle's.  tests/test_stream_order_table.py holds the scripts to being a check on the CPU.

All cases run in ONE fresh child process with GPU_MAX_HW_QUEUES=8 (tests/stream_order.py main): four hardware queues keep the context's
three streams and one caller's stream apart, but the stream-switch scripts need a second caller's stream, and in a process that has run the
rest of the suite the mapping of streams to queues is whatever the earlier tests left.  The cases here read the child's verdicts."""
import json
import os
import subprocess
import sys

import pytest

import stream_order as so

pytestmark = pytest.mark.gpu
LIMIT_S = 600


@pytest.fixture(scope="module")
def verdicts(gpu):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    run = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(so.__file__)], env=env, capture_output=True, text=True)
    out = {}
    for line in run.stdout.splitlines():
        if line.startswith("RESULT "):
            r = json.loads(line[7:])
            out[r["script"], r["placement"]] = r
    print("\n".join(l for l in run.stdout.splitlines() if l.startswith(("stream_order ", "TOTAL"))))
    return out, run


@pytest.mark.parametrize("placement", so.PLACEMENTS)
@pytest.mark.parametrize("script", so.SCRIPTS, ids=lambda s: s.name)
def test_script_behind_a_stalled_stream(script, placement, verdicts):
    out, run = verdicts
    r = out.get((script.name, placement))
    assert r is not None, ("the child process ended before this case", run.returncode, run.stderr[-1500:])
    assert r["ok"], r["message"]
