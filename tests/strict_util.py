"""What tests/test_strict_arithmetic.py runs its child processes with: the suite's own tests, or tests/strict_probe.py, on a build of
the kernels whose a*b+c round twice (-ffp-contract=off) -- the arithmetic of the reference's numpy scalars and of the C oracle --
next to the product, which contracts them (highwayenv_amd/build.py: FP_CONTRACT).

Which build a process runs is decided at import time (HWY_ENGINE_LIB: highwayenv_amd/_lib.py; HWY_EMU_FLAGS: tests/emu/emu.py), so
every run on the strict arithmetic is a child process, and no process loads two engine libraries.

* ``emu`` children: ``-m "not gpu"`` with ``HWY_EMU_FLAGS=-ffp-contract=off`` -- the emulator drivers build a library of their own
  per flag set (tests/emu/emu.py: flagged);
* ``hip`` children: ``-m gpu`` with ``HWY_ENGINE_LIB`` naming ``libhwy_engine_strict.so`` (highwayenv_amd/build.py:
  build_engine_strict), and the same HWY_EMU_FLAGS, so that the tests of a selection that hold the engine to the emulation
  compare two builds of ONE arithmetic.

GPU children run one after another under a time limit of their own.  After one of them ended with a fault -- its time limit, a
signal, or an illegal memory access in its output -- no further strict GPU child is started in this session: the remaining cases
fail at once with that reason (FAULT)."""
from __future__ import annotations

import os
import re
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRICT_EMU_FLAGS = "-ffp-contract=off"
# (what selects a build or narrows a run, taken out of a child's environment before its own settings go in)
_KNOBS = ("HWY_ENGINE_LIB", "HWY_EMU_FLAGS", "HWY_STRICT_TOL", "HWY_FUZZ_BACKEND", "HWY_FUZZ_FIRST", "HWY_FUZZ_CHUNKS", "HWY_FUZZ_CALIBRATE",
          # a prebuilt (mutated) emulator library named to one of the drivers of tests/emu would be run in place of the strict build
          "HWY_EMU_LIB", "HWY_EMU_TRAFFIC_LIB", "HWY_EMU_CONTROL_LIB", "HWY_EMU_LIDAR_LIB", "HWY_EMU_TTC_LIB")
FAULT = None  # the reason no further strict GPU child is started in this session
FAULT_CODES = (134, 139, -6, -11)
FAULT_TEXT = "an illegal memory access"


def strict_library() -> str:
    """libhwy_engine_strict.so, rebuilt only if it is missing or older than a source (highwayenv_amd.build.is_stale's rule)."""
    from highwayenv_amd import build
    return build.build_engine_strict()


def child_env(backend: str, strict: bool, tol: bool = False, extra=None) -> dict:
    env = {k: v for k, v in os.environ.items() if k not in _KNOBS}
    if strict:
        env["HWY_EMU_FLAGS"] = STRICT_EMU_FLAGS
        if backend == "hip":
            env["HWY_ENGINE_LIB"] = strict_library()
    if tol:
        env["HWY_STRICT_TOL"] = "1"
    env.update(extra or {})
    return env


def run_child(backend: str, argv, env: dict, timeout: float) -> subprocess.CompletedProcess:
    """`argv` (after the interpreter) in a child process, killed at `timeout` seconds.  A ``hip`` child that faults ends the strict
    GPU runs of the session (module docstring); the child that faulted fails here, with what it printed."""
    global FAULT
    gpu = backend == "hip"
    if gpu and FAULT:
        raise AssertionError(f"not started: an earlier strict GPU child faulted ({FAULT})")
    # a session of its own: at the time limit the child AND whatever it started (a selection's tests start processes) are killed
    proc = subprocess.Popen([sys.executable, *argv], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                            start_new_session=True)
    try:
        out, err = proc.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(proc.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        out, err = proc.communicate()
        if gpu:
            FAULT = f"{' '.join(argv[:6])} ...: no end after {timeout:.0f} s"
        raise AssertionError(f"child killed at its time limit of {timeout:.0f} s: {' '.join(argv)}\n{(out or '')[-3000:]}") from None
    res = subprocess.CompletedProcess(proc.args, proc.returncode, out, err)
    if gpu and (res.returncode in FAULT_CODES or FAULT_TEXT in res.stdout or FAULT_TEXT in res.stderr):
        FAULT = f"{' '.join(argv[:6])} ...: return code {res.returncode}"
        raise AssertionError(f"strict GPU child faulted (return code {res.returncode}): {' '.join(argv)}\n"
                             f"{res.stdout[-3000:]}\n{res.stderr[-2000:]}")
    return res


def run_selection(backend: str, selection, strict: bool = True, tol: bool = False, extra_env=None, timeout: float = 600,
                  marker: str | None = None) -> subprocess.CompletedProcess:
    """pytest `selection` in a child on `backend` ("emu": -m "not gpu"; "hip": -m gpu), on the strict build or on the product;
    `tol`: with HWY_STRICT_TOL=1 (tests/golden_util.py).  -s: what the selected tests print is in the child's stdout."""
    marker = marker or ("gpu" if backend == "hip" else "not gpu")
    argv = ["-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", "-p", "no:xdist", "-m", marker, *selection]
    return run_child(backend, argv, child_env(backend, strict, tol, extra_env), timeout)


def passed_count(res: subprocess.CompletedProcess) -> int:
    m = re.search(r"(\d+) passed", res.stdout)
    return int(m.group(1)) if m else 0


def assert_all_passed(res: subprocess.CompletedProcess, what: str) -> int:
    """The child ran tests, and every one of them passed: none failed, none errored, none was skipped."""
    tail = f"{what} (return code {res.returncode}):\n{res.stdout[-4000:]}\n{res.stderr[-1500:]}"
    assert res.returncode == 0, tail
    n = passed_count(res)
    assert n > 0 and not re.search(r"\d+ (failed|error|errors|skipped|xfailed|xpassed)\b", res.stdout.splitlines()[-1]), tail
    return n
