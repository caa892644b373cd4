"""What tests/test_mutations.py and tests/test_control_mutations.py share: building a CPU emulator from a mutated COPY of the
kernel source, and running a selection of the suite against it in a subprocess."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")


def build_mutant(sites, driver: str, lib: str) -> str:
    """tests/emu/_build/`lib` from `driver` (a .cpp of tests/emu) over a copy of the sources in which every (file of
    highwayenv_amd/csrc, old, new) of `sites` is replaced -- each `old` must be found exactly once."""
    from tests.emu import emu
    src = os.path.join(BUILD, f"{lib}_{os.getpid()}.src")
    shutil.rmtree(src, ignore_errors=True)
    for d in ("tests/emu", "highwayenv_amd/csrc", "include"):
        os.makedirs(os.path.join(src, d))
        for f in os.listdir(os.path.join(ROOT, d)):
            if f.endswith((".h", ".cpp")):
                shutil.copy(os.path.join(ROOT, d, f), os.path.join(src, d, f))
    for fname, old, new in sites:
        path = os.path.join(src, "highwayenv_amd", "csrc", fname)
        text = open(path).read()
        assert text.count(old) == 1, f"mutation site of {lib} not found exactly once in {fname}: {old}"
        open(path, "w").write(text.replace(old, new))
    out = os.path.join(BUILD, lib)
    emu.compile_emulator(os.path.join(src, "tests", "emu", driver), out)
    shutil.rmtree(src)
    return out


def run_selection(lib, selection, env_var: str, env_extra=None) -> subprocess.CompletedProcess:
    """pytest `selection` in a subprocess whose emulator is `lib` (None: the suite's own), named to it by `env_var`."""
    env = dict(os.environ, **(env_extra or {}))
    env.pop(env_var, None)
    if lib:
        env[env_var] = lib
    return subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", *selection], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=1500)
