"""CPU: the contract of tests/_child.py.  The children are `python -c` one-liners that import neither torch nor the library and
never open a GPU; every test builds a fresh ChildRunner, so the process-wide instance is never latched by a test."""
import os
import signal
import subprocess
import sys
import time

import pytest

import _child
from _child import ChildRunner, json_lines, last_json

FAILED = pytest.fail.Exception


def _py(code, *args):
    return [sys.executable, "-c", code, *args]


def _touch(path):
    return _py("import sys; open(sys.argv[1], 'w').close()", str(path))


def _refused(r, marker):
    """the next run() fails with "not started" and creates no process"""
    with pytest.raises(FAILED, match="(?s)not started: .* ended with "):
        r.run(_touch(marker), limit=30)
    assert not os.path.exists(marker)


@pytest.mark.parametrize("code", [0, 3])
def test_an_ordinary_exit_does_not_latch(tmp_path, code):
    r = ChildRunner()
    p = r.run(_py("import sys; print('out'); print('err', file=sys.stderr); sys.exit(%d)" % code), limit=30)
    assert (p.returncode, p.stdout, p.stderr) == (code, "out\n", "err\n")
    assert r.latched is None and r.stopped == {}
    assert r.run(_touch(tmp_path / "m"), limit=30).returncode == 0 and os.path.exists(tmp_path / "m")


@pytest.mark.parametrize("code", [134, 139, 124, 137])
def test_a_fault_status_latches(tmp_path, code):
    r = ChildRunner()
    p = r.run(_py("import sys; sys.exit(%d)" % code), limit=30)
    assert p.returncode == code                               # the casualty's own test sees the return code, as before
    assert r.latched[1] == "return code %d" % code
    _refused(r, tmp_path / "m")


def test_a_child_that_ends_by_signal_latches(tmp_path):
    r = ChildRunner()
    p = r.run(_py("import os, signal; os.kill(os.getpid(), signal.SIGKILL)"), limit=30)
    assert p.returncode == -signal.SIGKILL
    _refused(r, tmp_path / "m")
    _refused(r, tmp_path / "m")                               # ... and stays latched, on the first casualty
    assert r.latched[1] == "return code -9"


def _alive(pid):
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return False
    with open("/proc/%d/stat" % pid) as f:                    # (a zombie waiting for init to reap it is gone for our purpose)
        return f.read().rsplit(")", 1)[1].split()[0] != "Z"


def test_the_time_limit_latches_and_takes_the_grandchild_along(tmp_path):
    pidfile = str(tmp_path / "pid")
    code = ("import subprocess, sys, time\n"
            "g = subprocess.Popen([sys.executable, '-c', 'import time; time.sleep(60)'])\n"
            "open(sys.argv[1] + '.tmp', 'w').write(str(g.pid)); __import__('os').rename(sys.argv[1] + '.tmp', sys.argv[1])\n"
            "time.sleep(60)\n")
    r = ChildRunner()
    with pytest.raises(subprocess.TimeoutExpired):
        r.run(_py(code, pidfile), limit=1)
    assert r.latched[1] == "its 1 s time limit"
    pid = int(open(pidfile).read())
    for _ in range(100):                                      # killed already; init may take a moment to reap it
        if not _alive(pid):
            break
        time.sleep(0.05)
    assert not _alive(pid)
    _refused(r, tmp_path / "m")


def _run_from(filename, r, argv, **kw):
    """r.run(argv, **kw) called from code whose file name is ``filename``"""
    scope = dict(r=r, argv=argv, kw=kw)
    exec(compile("p = r.run(argv, **kw)", filename, "exec"), scope)
    return scope["p"]


def test_stop_file_on_failure_stops_that_file_alone(tmp_path):
    r = ChildRunner()
    p = _run_from("test_a.py", r, _py("import sys; sys.exit(3)"), limit=30, stop_file_on_failure=True)
    assert p.returncode == 3 and r.latched is None
    with pytest.raises(FAILED, match="(?s)not started: .* ended with return code 3"):
        _run_from("test_a.py", r, _touch(tmp_path / "a"), limit=30, stop_file_on_failure=True)
    assert not os.path.exists(tmp_path / "a")
    assert _run_from("test_b.py", r, _touch(tmp_path / "b"), limit=30, stop_file_on_failure=True).returncode == 0
    assert os.path.exists(tmp_path / "b")
    # without the flag an exit of 3 stops nothing
    r = ChildRunner()
    _run_from("test_a.py", r, _py("import sys; sys.exit(3)"), limit=30)
    assert _run_from("test_a.py", r, _touch(tmp_path / "c"), limit=30).returncode == 0


def _child_environ(r, **kw):
    p = r.run(_py("import os, json; print(json.dumps(dict(os.environ)))"), limit=30, **kw)
    return last_json(p)


def test_the_child_gets_the_environment_the_old_code_built(monkeypatch):
    for k, v in (("A", "1"), ("B", "2"), ("C", "3"), ("EC_AMD_LIB", "/x/lib.so"), ("EC_CONV_BIG", "4"), ("EC_POLICY_FAST", "0")):
        monkeypatch.setenv(k, v)
    r = ChildRunner()
    # the switch-setting tests: the module's switches removed, the setting laid over the rest
    switches, setting = ("A", "B"), {"B": "7", "D": "8"}
    env = {k: v for k, v in os.environ.items() if k not in switches}
    env.update(setting)
    assert _child_environ(r, drop=switches, env=setting) == env
    assert env["B"] == "7" and "A" not in env and env["C"] == "3"
    # the act / learn routes: every EC_ variable but EC_AMD_LIB removed
    env = {k: v for k, v in os.environ.items() if not k.startswith("EC_") or k == "EC_AMD_LIB"}
    env.update({"EC_POLICY_FAST": "1"})
    assert _child_environ(r, drop="EC_*", env={"EC_POLICY_FAST": "1"}) == env
    assert env["EC_AMD_LIB"] == "/x/lib.so" and "EC_CONV_BIG" not in env
    # the rest: the parent's environment, with or without one variable over it
    assert _child_environ(r, env={"EC_RN50_FUSE": "0"}) == {**os.environ, "EC_RN50_FUSE": "0"}
    assert _child_environ(r) == dict(os.environ)
    assert _child.child_env() == dict(os.environ)


def test_cwd_and_input_reach_the_child(tmp_path):
    p = ChildRunner().run(_py("import os, sys; print(os.getcwd()); print(sys.stdin.read())"), limit=30, cwd=str(tmp_path), input="fed")
    assert p.stdout.split() == [os.path.realpath(tmp_path), "fed"]


def _done(stdout, stderr="", rc=0):
    return subprocess.CompletedProcess(["x"], rc, stdout, stderr)


def test_last_json_and_json_lines():
    p = _done('note\n{"a": 1}\nnot json {\n{"b": 2}\n\n')
    assert last_json(p) == {"b": 2}
    assert json_lines(p) == [{"a": 1}, {"b": 2}]
    for bad in (_done("", "Traceback: boom", 1), _done("only words\n", "Traceback: boom", 1)):
        with pytest.raises(AssertionError, match="Traceback: boom"):
            last_json(bad)
        with pytest.raises(AssertionError, match="Traceback: boom"):
            json_lines(bad)
