"""GPU: every kernel-selecting environment knob, each group in a fresh process.

mvx_ops.hip (config(), into the Config of mvx_ops_tab.h) and mvx_pack.hip read
their knobs once, so a knob can only be tested in a process that starts with
it set.
tests/knob_worker.py holds the groups (its ENV) and the checks; here one
worker runs at a time, each under its own time limit, with the parent's
environment plus the group's knobs.  A worker that ends by a signal, an
abort or its time limit fails its test and the groups after it are skipped,
not started.
"""
import os
import subprocess
import sys

import pytest

import knob_worker

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "knob_worker.py")
_died = []          # the group whose process died; nothing is started after it


def test_at_most_six_processes_and_every_knob_in_one():
    knobs = ["MVX_PROG_U", "MVX_PROG_GENERIC", "MVX_PROG4", "MVX_CHAIN_RT", "MVX_NO_BODY", "MVX_NT_MIN_BYTES",
             "MVX_BLOCK_CAP", "MVX_CAP_APPLY", "MVX_CAP_PROG", "MVX_CAP_TREE", "MVX_PXI_U", "MVX_PXI_CAP",
             "MVX_PXI_APPLY_CAP", "MVX_UNPACK_MERGE", "MVX_UNPACK_CHUNK_TAB", "MVX_LDS_SWIZZLE", "MVX_PACK_TILES",
             "MVX_PACK_CHUNK_TAB", "MVX_PACK_UNITS"]
    assert len(knob_worker.ENV) <= 6
    for k in knobs:
        assert sum(k in env for env in knob_worker.ENV.values()) == 1, k


@pytest.mark.parametrize("group", list(knob_worker.ENV))
def test_knob_group(group):
    if _died:
        pytest.skip("the knob process of group %r died; no further process is started" % _died[0])
    env = dict(os.environ)
    env.update(knob_worker.ENV[group])
    try:
        r = subprocess.run([sys.executable, WORKER, group], env=env, timeout=knob_worker.TIMEOUT[group],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        _died.append(group)
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail("group %s ran into its %d s limit; last output:\n%s" % (group, knob_worker.TIMEOUT[group],
                                                                           out[-3000:]))
    tail = r.stdout[-3000:]
    if r.returncode < 0 or r.returncode in (134, 137, 139):
        _died.append(group)
        pytest.fail("group %s died (exit status %d); last output:\n%s" % (group, r.returncode, tail))
    assert r.returncode == 0, "group %s failed (exit status %d):\n%s" % (group, r.returncode, tail)
    lines = r.stdout.strip().splitlines()
    last = lines[-1].split() if lines else []
    assert len(last) == 4 and last[:2] == ["knobs", "ok"] and last[3] == "checks" and int(last[2]) > 0, tail
    assert int(last[2]) == sum(ln.startswith("ok ") for ln in lines), tail
