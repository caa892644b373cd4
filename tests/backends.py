"""Backends the parity tests run against.

* ``emu``  -- the product's kernel SOURCE executed on the CPU by tests/emu (no GPU needed);
* ``hip``  -- the product itself: libhwy_engine.so on a real MI355X through the C-ABI.

Either is ONE engine class for every configuration: the product's ``Engine``, the emulation's ``EmuEngine`` (tests/emu/emu.py).
"""
import pytest


def make_engine(backend: str, cfg):
    if backend == "emu":
        from tests.emu.emu import EmuEngine
        return EmuEngine(cfg)
    from highwayenv_amd.engine import Engine
    return Engine(cfg)


def emu_class(base):
    """`base` (a Batched*Env or a single-environment drop-in) on the CPU emulation of the kernels."""
    from tests.emu.emu import EmuEngine
    return type("Emu" + base.__name__, (base,), {"_engine_factory": staticmethod(lambda cfg, device, stream: EmuEngine(cfg))})


def env_class(backend: str, base):
    """`base` on the backend: the tests substitute the CPU emulation of the same kernel source."""
    return emu_class(base) if backend == "emu" else base


BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
