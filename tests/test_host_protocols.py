"""CPU: the two host-side protocols that let several scenes in flight share one model -- _lib.build_once (shared
artefacts built once, published, stored in one assignment) and occ_decoder.run_with_range_fallback (the decoder's
f16-range flag answered by a re-run at the fallback scale).  The status word, the runs and the decoder are stubs."""
import contextlib
import threading
import time
import types

import numpy as np
import pytest
import torch

from rfdnet_amd import _lib
from rfdnet_amd.iscnet.occ_decoder import run_with_range_fallback


# ---------------------------------------------------------------------------------------------------- build_once ----
def test_build_once_builds_once_for_eight_threads_released_together():
    store, built, out, go = {}, [], [None] * 8, threading.Barrier(8)

    def build():
        built.append(1)
        time.sleep(0.05)                       # the other seven threads arrive while this one builds
        return object()

    def work(i):
        go.wait()
        out[i] = _lib.build_once(store, "slot", ("k", 1), build, torch.device("cpu"))
    ts = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert len(built) == 1 and all(o is out[0] for o in out)
    assert store == {"slot": (("k", 1), out[0])}


def test_build_once_rebuilds_on_a_changed_key_and_a_slot_keeps_one_entry():
    store, cpu = {}, torch.device("cpu")
    a = _lib.build_once(store, "slot", 1, lambda: ["a"], cpu)
    assert _lib.build_once(store, "slot", 1, lambda: ["b"], cpu) is a          # same key: the stored value
    b = _lib.build_once(store, "slot", 2, lambda: ["b"], cpu)
    assert b == ["b"] and b is not a and list(store) == ["slot"] and store["slot"] == (2, b)


def test_build_once_clears_a_multi_entry_store_above_its_limit():
    store, cpu = {}, torch.device("cpu")
    for k in range(4):
        _lib.build_once(store, k, k, lambda: k, cpu, limit=3)
    assert sorted(store) == [0, 1, 2, 3]                                       # up to limit + 1 entries
    assert _lib.build_once(store, 2, 2, lambda: "new", cpu, limit=3) == 2      # a hit neither builds nor clears
    assert len(store) == 4
    assert _lib.build_once(store, 4, 4, lambda: 4, cpu, limit=3) == 4          # the next miss clears, then stores
    assert store == {4: (4, 4)}


def test_build_once_publishes_only_on_a_cuda_device(monkeypatch):
    published = []
    monkeypatch.setattr(_lib, "publish", published.append)
    _lib.build_once({}, "slot", 1, lambda: 0, torch.device("cpu"))
    assert published == []
    _lib.build_once({}, "slot", 1, lambda: 0, torch.device("cuda", 0))      # (publish is a stub: no GPU needed)
    assert published == [torch.device("cuda", 0)]


# -------------------------------------------------------------------------------------- run_with_range_fallback ----
class Dec(object):
    """the decoder as run_with_range_fallback sees it: a scale 2^ka (6, fallback 3) and lower_activation_scale()"""

    def __init__(self, ka=6):
        self.ka = ka

    def lower_activation_scale(self):
        if self.ka <= 3:
            return False
        self.ka = 3
        return True


@pytest.fixture
def stub_status(monkeypatch):
    """-> set(statuses): the words stream_status_bits() returns one by one; torch.cuda.device is a no-op"""
    seq = []
    monkeypatch.setattr(_lib, "stream_status_bits", lambda: seq.pop(0))
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())

    def set_(statuses):
        seq[:] = statuses
        return seq
    return set_


def recorder(dec, other_scene_lowers=False):
    runs = []

    def run():
        runs.append(dec.ka)
        if other_scene_lowers and len(runs) == 1:
            dec.ka = 3                      # another host thread answers ITS flag while this run is in flight
        return "out@%d" % runs[-1]
    return run, runs


def test_fallback_flag_then_clean_reruns_once_at_the_fallback_scale(stub_status):
    dec = Dec()
    run, runs = recorder(dec)
    left = stub_status([2, 0])
    assert run_with_range_fallback(dec, run, None) == "out@3"
    assert runs == [6, 3] and dec.ka == 3 and left == []


def test_fallback_clean_runs_once(stub_status):
    dec = Dec()
    run, runs = recorder(dec)
    stub_status([0])
    assert run_with_range_fallback(dec, run, None) == "out@6" and runs == [6] and dec.ka == 6


def test_fallback_flag_at_the_fallback_scale_raises_after_one_run(stub_status):
    dec = Dec(ka=3)
    run, runs = recorder(dec)
    stub_status([2])
    with pytest.raises(_lib.RfdHipError, match="occupancy decoder"):
        run_with_range_fallback(dec, run, None)
    assert runs == [3]


def test_fallback_flag_twice_raises_after_two_runs(stub_status):
    dec = Dec()
    run, runs = recorder(dec)
    stub_status([2, 2])
    with pytest.raises(_lib.RfdHipError, match="occupancy decoder"):
        run_with_range_fallback(dec, run, None)
    assert runs == [6, 3]


def test_fallback_reruns_when_another_scene_lowered_the_scale_during_the_run(stub_status):
    dec = Dec()
    run, runs = recorder(dec, other_scene_lowers=True)
    stub_status([2, 0])
    assert run_with_range_fallback(dec, run, None) == "out@3" and runs == [6, 3]


def test_fallback_rerun_answers_only_the_range_flag(stub_status):
    """the re-run answers bit 2; another flag of the first run (bit 1: FPS abort) still raises"""
    dec = Dec()
    run, runs = recorder(dec)
    stub_status([3, 0])
    with pytest.raises(_lib.RfdHipError, match="furthest point sampling") as e:
        run_with_range_fallback(dec, run, None)
    assert e.value.status == 1 and runs == [6, 3]


def test_fallback_flags_of_earlier_stages_come_first(stub_status):
    """before() raising: its exception, no re-run, and the decoder's scale is left alone"""
    class Earlier(Exception):
        pass

    def before():
        raise Earlier()
    dec = Dec()
    run, runs = recorder(dec)
    stub_status([2])
    with pytest.raises(Earlier):
        run_with_range_fallback(dec, run, None, before=before)
    assert runs == [6] and dec.ka == 6


def test_estimate_normals_reruns_when_the_scale_came_down_while_it_folded(stub_status):
    """Generator3D.estimate_normals reads the scale BEFORE it folds: a fold that ran while another scene lowered the
    shared decoder's scale (the stub's first fold) is answered by a re-run, not by a spurious range error."""
    from rfdnet_amd.iscnet.generator import Generator3D

    class FoldDec(Dec):
        def __init__(self):
            super().__init__(ka=6)
            self.folds, self.runs = 0, []

        def fold(self, z, c):
            self.folds += 1
            if self.folds == 1:
                self.ka = 3                 # another scene lowers the scale while this call folds
            return ("table", self.ka), "fc_p_w"

        def normals(self, v, vend, table, fc_p_w):
            self.runs.append(table[1])
            return torch.full((v.shape[0], 3), float(table[1]))

    dec = FoldDec()
    left = stub_status([2, 0])
    gen = Generator3D(types.SimpleNamespace(decoder=dec))
    nrm = gen.estimate_normals(np.zeros((5, 3)), torch.zeros(4), torch.zeros(8), device="cpu")
    assert dec.runs == [3, 3] and dec.folds == 2 and left == []
    assert nrm.shape == (5, 3) and (nrm == 3).all()
