"""The one place a `gpu` test starts a process (the library reads its EC_* switches once per process, so a test of a switch setting
needs a process of its own).  Every tests/test_gpu_*.py goes through the module-level ``GPU = ChildRunner()``:

    p = GPU.run([sys.executable, script, setting], drop=R.SWITCHES, env=R.SETTINGS[setting], limit=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    res = last_json(p)

The latch.  After a child that ended by signal, with 134 (abort), 139 (segmentation fault), 124 or 137 (a time limit inside it), or
at its own ``limit``, the card may be faulted or still held: nothing more is started on it in this pytest process.  The test whose
child ended so fails as any test with a failed child does (its return code is asserted; TimeoutExpired is re-raised); every later
run(), from whichever test file, fails its test with "not started: ..." before it creates a process.

``stop_file_on_failure=True`` (the act-route and learn-route tests): any non-zero exit, or the time limit, also stops the later
run() calls made from the same test file -- one wrong route there makes the other settings' figures meaningless, not dangerous.

The child is the leader of a session of its own; at ``limit`` its whole process group is killed and reaped, so that a child's own
children (bench.py --gpus N starts one per GPU) do not outlive it with the GPU open.

In-process GPU tests are not gated by the latch: skipping them would take a collection hook in conftest.py.  CPU-side children
(the recorder runs of tests/test_*_cabi.py, tests/golden/make_*.py) never open a GPU and do not come through here."""
import json
import os
import signal
import subprocess
import sys

import pytest

DEADLY = (134, 139, 124, 137)          # abort, segmentation fault, `timeout`'s own two


def child_env(env=None, drop=()):
    """os.environ without the names in ``drop`` ("EC_*": without every EC_ variable but EC_AMD_LIB), then ``env`` laid over it"""
    if drop == "EC_*":
        out = {k: v for k, v in os.environ.items() if not k.startswith("EC_") or k == "EC_AMD_LIB"}
    else:
        out = {k: v for k, v in os.environ.items() if k not in drop}
    out.update(env or {})
    return out


def _tail(p):
    return "return code %s; stdout ends %r; stderr ends %r" % (p.returncode, p.stdout[-500:], p.stderr[-2000:])


def last_json(p):
    """the last stdout line of a finished child, as JSON"""
    lines = p.stdout.strip().splitlines()
    assert lines, "the child printed nothing: " + _tail(p)
    try:
        return json.loads(lines[-1])
    except ValueError:
        raise AssertionError("the child's last line is no JSON: " + _tail(p)) from None


def json_lines(p):
    """every stdout line of a finished child that starts with `{`, as JSON"""
    got = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    assert got, "the child printed no JSON line: " + _tail(p)
    return got


class ChildRunner:
    def __init__(self):
        self.latched = None            # (argv, how it ended) of the first casualty: set once, read by every later run()
        self.stopped = {}              # test file -> (argv, how it ended), under stop_file_on_failure

    def run(self, argv, *, env=None, drop=(), limit, cwd=None, input=None, stop_file_on_failure=False):
        """Start ``argv`` under child_env(env, drop), wait at most ``limit`` seconds -> subprocess.CompletedProcess (text output)."""
        caller = sys._getframe(1).f_code.co_filename
        first = self.latched or self.stopped.get(caller)
        if first:
            pytest.fail("not started: %s ended with %s" % first)
        who = " ".join(argv)[:300]
        with subprocess.Popen(argv, env=child_env(env, drop), cwd=cwd, stdin=subprocess.PIPE if input is not None else None,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True) as p:
            try:
                out, err = p.communicate(input, timeout=limit)
            except BaseException as e:                       # the time limit, or an interrupt of the suite: leave nothing behind
                try:
                    os.killpg(p.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                p.wait()
                if isinstance(e, subprocess.TimeoutExpired):
                    self.latched = (who, "its %d s time limit" % limit)
                raise
        if p.returncode < 0 or p.returncode in DEADLY:
            self.latched = (who, "return code %d" % p.returncode)
        elif stop_file_on_failure and p.returncode != 0:
            self.stopped[caller] = (who, "return code %d" % p.returncode)
        return subprocess.CompletedProcess(argv, p.returncode, out, err)


GPU = ChildRunner()
