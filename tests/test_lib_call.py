"""CPU: the call boundary of the host modules -- _lib.ABI / bind() (one table of the C ABI; only the test hooks may be
absent from a library), _lib.call() / ptr() (the one launcher) and build.py's stamp of the RFD_NO_TEST_HOOKS setting.
The library, its functions, the stream and the compiler are stubs: nothing is built and no GPU is touched."""
import contextlib
import ctypes
import os
import types

import pytest
import torch

from rfdnet_amd import _lib, build

HOOKS = ("rfd_test_hold_cus", "rfd_fps_test_phantom_units")


def stub_library(without=()):
    """an object with a function (returning 0, recording its arguments in .calls) for every ABI entry but `without`"""
    stub = types.SimpleNamespace(calls=[])

    def make(name):
        def fn(*args):
            stub.calls.append((name, args))
            return 0
        return fn
    for name in _lib.ABI:
        if name not in without:
            setattr(stub, name, make(name))
    return stub


# ------------------------------------------------------------------------------------------------------ the table ----
def test_only_the_two_test_hooks_are_optional():
    assert sorted(n for n, e in _lib.ABI.items() if _lib.OPTIONAL in e[2:]) == sorted(HOOKS)
    assert _lib.exported_symbols() == sorted(_lib.ABI)
    assert all(_lib.SIGNATURES[n] is e[1] for n, e in _lib.ABI.items())


def test_bind_gives_every_entry_the_types_of_the_table():
    stub = _lib.bind(stub_library())
    for name, entry in _lib.ABI.items():
        fn = getattr(stub, name)
        assert fn.restype is entry[0] and fn.argtypes is entry[1], name
    assert stub.rfd_occ_decode_w8.restype is ctypes.c_int and stub.rfd_occ_packed_bytes.restype is ctypes.c_size_t
    assert stub.rfd_last_error_string.restype is ctypes.c_char_p and stub.rfd_last_error_string.argtypes == []


def test_bind_accepts_a_library_without_the_hooks_and_a_call_of_one_says_why():
    stub = _lib.bind(stub_library(without=HOOKS))
    assert stub.rfd_occ_decode_w8(1, 2) == 0                     # everything else is bound and callable
    for hook in HOOKS:
        with pytest.raises(_lib.RfdHipError, match="RFD_NO_TEST_HOOKS") as e:
            getattr(stub, hook)(0)
        assert hook in str(e.value)


def test_bind_names_a_missing_required_symbol_and_the_library():
    with pytest.raises(_lib.RfdHipError) as e:
        _lib.bind(stub_library(without=("rfd_occ_decode_w8",)))
    assert "rfd_occ_decode_w8" in str(e.value) and _lib.LIB_PATH in str(e.value)
    stub = stub_library(without=("rfd_occ_decode_w8",))
    stub._name = "/somewhere/else/librfd_hip.so"                  # ctypes.CDLL keeps its path there
    with pytest.raises(_lib.RfdHipError, match="/somewhere/else/librfd_hip.so"):
        _lib.bind(stub)


# ------------------------------------------------------------------------------------------------------- call, ptr ----
@pytest.fixture
def launcher(monkeypatch):
    """_lib.call() on a stub library, stream 0x5eed, with the devices it entered in .devices"""
    stub = _lib.bind(stub_library())
    stub.devices = []

    @contextlib.contextmanager
    def device(dev):
        stub.devices.append(dev)
        yield
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    monkeypatch.setattr(_lib, "current_stream", lambda: 0x5eed)
    monkeypatch.setattr(torch.cuda, "device", device)
    return stub


def test_call_passes_the_arguments_then_the_stream_on_the_device(launcher):
    a, b, dev = object(), object(), torch.device("cuda", 1)
    assert _lib.call("rfd_mise_count", dev, a, None, b) is None
    assert launcher.calls == [("rfd_mise_count", (a, None, b, 0x5eed))]
    assert launcher.devices == [dev]


def test_a_failed_call_names_the_entry_point_that_ran(launcher):
    launcher.rfd_occ_decode_w8 = lambda *args: 1
    launcher.rfd_last_error_string = lambda: b"invalid argument"
    with pytest.raises(_lib.RfdHipError) as e:
        _lib.call("rfd_occ_decode_w8", torch.device("cuda", 0), 8)
    assert "rfd_occ_decode_w8 failed" in str(e.value) and "invalid argument" in str(e.value)
    _lib.call("rfd_occ_decode", torch.device("cuda", 0), 8)       # the other entry point still succeeds


def test_ptr():
    t = torch.zeros(3)
    assert _lib.ptr(None) is None and _lib.ptr(t) == t.data_ptr() != 0


# --------------------------------------------------------------------------------------------------- build's stamp ----
@pytest.mark.parametrize("first, second", [(None, "1"), ("1", None), ("1", "0")])
def test_the_library_is_stale_under_the_other_hook_setting(tmp_path, monkeypatch, first, second):
    commands = []

    def compiler(cmd):
        commands.append(cmd)
        open(cmd[cmd.index("-o") + 1], "w").close()

    def setting(value):
        if value is None:
            monkeypatch.delenv("RFD_NO_TEST_HOOKS", raising=False)
        else:
            monkeypatch.setenv("RFD_NO_TEST_HOOKS", value)
    monkeypatch.setattr(build, "LIB_DIR", str(tmp_path))
    monkeypatch.setattr(build, "LIB_PATH", str(tmp_path / "librfd_hip.so"))
    monkeypatch.setattr(build, "STAMP_PATH", str(tmp_path / "librfd_hip.stamp"))
    monkeypatch.setattr(build.subprocess, "check_call", compiler)
    setting(first)
    assert build.is_stale()                                       # nothing there yet
    build.build()
    assert len(commands) == 1 and ("-DRFD_NO_TEST_HOOKS" in commands[0]) == (first == "1")
    assert not build.is_stale()
    setting(second)
    assert build.is_stale()
    build.build()
    assert len(commands) == 2 and ("-DRFD_NO_TEST_HOOKS" in commands[1]) == (second == "1")
    assert not build.is_stale()
    setting(first)
    assert build.is_stale()


def test_a_library_without_a_stamp_is_stale(tmp_path, monkeypatch):
    monkeypatch.setattr(build, "LIB_PATH", str(tmp_path / "librfd_hip.so"))
    monkeypatch.setattr(build, "STAMP_PATH", str(tmp_path / "librfd_hip.stamp"))
    open(build.LIB_PATH, "w").close()
    assert build.is_stale()
    with open(build.STAMP_PATH, "w") as f:
        f.write(build._stamp())
    assert not build.is_stale() and os.path.exists(build.LIB_PATH)


# ------------------------------------------------------------------------------------------------------ the guard ----
def test_need_gpu_refuses_whatever_is_no_device_tensor():
    import numpy as np
    _lib.need_gpu()
    for bad in (torch.zeros(2), np.zeros(2), None):
        with pytest.raises(RuntimeError, match="CPU not supported"):
            _lib.need_gpu(bad)
    meta = types.SimpleNamespace(device=types.SimpleNamespace(type='cuda'))    # looks like one, is no tensor
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _lib.need_gpu(meta)
