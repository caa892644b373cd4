"""The action-mask entry points are additive to ABI v8: the version and the struct sizes stay, the two exports exist and are
declared in the public header, and a NULL engine is refused."""
import ctypes as C
import os
import re

import pytest

from highwayenv_amd import _abi, _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hwy_engine.h")


def test_sizes_and_version_unchanged():
    assert _abi.HWY_ABI_VERSION == 8
    assert C.sizeof(_abi.HwyConfig) == 6304
    assert C.sizeof(_abi.HwyOpdParams) == 32
    text = open(HEADER).read()
    assert re.search(r"#define\s+HWY_ABI_VERSION\s+8\b", text)


def test_exports_declared_and_present():
    text = open(HEADER).read()
    lib = _lib.load()
    for name in ("hwy_action_mask_device", "hwy_action_mask"):
        assert name in _lib.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(\s*hwy_engine\s*\*\s*eng\s*,\s*uint8_t\s*\*" % name, text), name
        assert getattr(lib, name) is not None
    assert lib.hwy_config_size() == 6304 and lib.hwy_abi_version() == 8


def test_null_engine_is_invalid_arg():
    lib = _lib.load()
    buf = (C.c_uint8 * 16)()
    assert lib.hwy_action_mask(None, buf) == _abi.HWY_ERR_INVALID_ARG
    assert lib.hwy_action_mask_device(None, buf) == _abi.HWY_ERR_INVALID_ARG


@pytest.mark.gpu
def test_null_pointer_and_direct_control_on_an_engine():
    from highwayenv_amd.engine import Engine, EngineError
    eng = Engine(_abi.make_config(_abi.highway_fast_default_config(), 2, fast=True))
    lib = _lib.load()
    assert lib.hwy_action_mask(eng._h, None) == _abi.HWY_ERR_INVALID_ARG
    assert lib.hwy_action_mask_device(eng._h, None) == _abi.HWY_ERR_INVALID_ARG
    with pytest.raises(EngineError):
        eng.action_mask_device(0)
    direct = Engine(_abi.make_config(dict(_abi.highway_fast_default_config(), action={"type": "DiscreteAction"}), 2, fast=True))
    buf = (C.c_uint8 * 64)()
    assert lib.hwy_action_mask(direct._h, buf) == _abi.HWY_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        direct.action_mask()
