"""CPU: the two host-side protocols that let several scenes in flight share one model -- _lib.build_once (shared
artefacts built once, published, stored in one assignment; _lib.ArtefactCache: bounded, evicting one entry after a device
synchronise; _lib.tensor_key) and occ_decoder.run_with_range_fallback (the decoder's
f16-range flag answered by a re-run at the fallback scale).  The status word, the runs and the decoder are stubs."""
import contextlib
import gc
import threading
import time
import types
import weakref

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


def test_build_once_publishes_only_on_a_cuda_device(monkeypatch):
    published = []
    monkeypatch.setattr(_lib, "publish", published.append)
    _lib.build_once({}, "slot", 1, lambda: 0, torch.device("cpu"))
    assert published == []
    _lib.build_once({}, "slot", 1, lambda: 0, torch.device("cuda", 0))      # (publish is a stub: no GPU needed)
    assert published == [torch.device("cuda", 0)]


# ------------------------------------------------------------------------------------------------ ArtefactCache ----
class Artefact(object):
    """a value a weakref can watch (what a cached device tensor is to the allocator)"""

    def __init__(self, k):
        self.k = k


@pytest.fixture
def events(monkeypatch):
    """-> the list that the stubs of publish / sync_device append ("publish" | "sync", device) to: no GPU needed"""
    log = []
    monkeypatch.setattr(_lib, "publish", lambda d: log.append(("publish", d)))
    monkeypatch.setattr(_lib, "sync_device", lambda d: log.append(("sync", d)))
    return log


def test_artefact_cache_evicts_the_oldest_entry_only(events):
    cache, cpu, built = _lib.ArtefactCache(3), torch.device("cpu"), []

    def get(k):
        return cache.get(k, lambda: built.append(k) or Artefact(k), cpu)
    seen = []
    for k in range(5):
        assert get(k).k == k
        seen.append(list(cache.store))
    assert seen == [[0], [0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 4]]              # one eviction per miss: 0, then 1
    assert get(3).k == 3 and get(2).k == 2                                     # a hit neither builds nor evicts
    assert built == [0, 1, 2, 3, 4] and list(cache.store) == [2, 3, 4]
    assert get(0).k == 0 and list(cache.store) == [3, 4, 0]                    # least recently BUILT: the hit on 2 did
    assert built == [0, 1, 2, 3, 4, 0]                                         # not save it; an evicted key is rebuilt
    assert events == []                                                        # cpu: nothing published, nothing waited for


def test_artefact_cache_synchronises_the_device_before_it_drops_an_evicted_value(events):
    cache, dev, refs = _lib.ArtefactCache(2), torch.device("cuda", 0), []
    for k in range(3):
        if k == 2:
            assert events == [("publish", dev)] * 2                            # below the limit: waits for nothing
        refs.append(weakref.ref(cache.get(k, lambda: Artefact(k), dev), lambda _, k=k: events.append(("dropped", k))))
        assert cache.get(k, lambda: None, dev) is refs[k]()                    # a hit
    gc.collect()
    # one wait per eviction, BEFORE the value goes, and before the new entry is published and stored
    assert events[2:] == [("sync", dev), ("dropped", 0), ("publish", dev)] and list(cache.store) == [1, 2]
    del events[:]
    cache.get(3, lambda: Artefact(3), torch.device("cpu"))                     # the EVICTED entry's device decides
    assert events == [("sync", dev), ("dropped", 1)] and refs[1]() is None and refs[2]() is not None


def test_artefact_cache_keeps_its_key_tensors_alive(events):
    cache, cpu = _lib.ArtefactCache(1), torch.device("cpu")
    w = torch.zeros(4)
    ref = weakref.ref(w)
    cache.get(_lib.tensor_key(w), lambda: "packed", cpu, keep=w)
    del w
    gc.collect()
    assert ref() is not None                              # cached under its address: it must not be given out again
    cache.get("other", lambda: "x", cpu)
    gc.collect()
    assert ref() is None


def test_artefact_cache_builds_once_for_eight_threads_released_together(events):
    cache, built, out, go = _lib.ArtefactCache(4), [], [None] * 8, threading.Barrier(8)

    def build():
        built.append(1)
        time.sleep(0.05)                       # the other seven threads arrive while this one builds
        return object()

    def work(i):
        go.wait()
        out[i] = cache.get(("k", 1), build, torch.device("cpu"))
    ts = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert len(built) == 1 and all(o is out[0] for o in out) and list(cache.store) == [("k", 1)]


def test_artefact_cache_under_eviction_hands_every_thread_its_own_value(events):
    """eight threads, eight keys, room for four: whatever is evicted meanwhile, get() returns what ITS build() made"""
    cache, bad, go = _lib.ArtefactCache(4), [], threading.Barrier(8)

    def work(i):
        go.wait()
        for n in range(200):
            k = (i + n) % 8
            v = cache.get(k, lambda: ("made for", k), torch.device("cuda", 0), keep=k)
            if v != ("made for", k) or len(cache.store) > 4:
                bad.append((i, n, v, len(cache.store)))
    ts = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert bad == [] and len(cache.store) == 4
    assert all(e == (k, ((("made for", k), k), torch.device("cuda", 0))) for k, e in cache.store.items())


def test_tensor_key():
    a = torch.zeros(3, 2)
    b = torch.zeros(3, 2)
    k = _lib.tensor_key(a, None, b)
    assert len(k) == 3 and k[1] is None and k == _lib.tensor_key(a, None, b)
    assert k[0] == (a.data_ptr(), a._version, (3, 2), torch.device("cpu"))
    assert k[0] != k[2]                                   # equal values at another address
    assert _lib.tensor_key(a.view(2, 3)) != k[:1]         # the shape is part of it
    a.add_(1)
    assert _lib.tensor_key(a) != k[:1] and _lib.tensor_key(b) == k[2:]         # an in-place write: _version
    assert _lib.tensor_key() == () and _lib.tensor_key(None) == (None,)


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


# ------------------------------------------------------------------------------------------------------ _lib.rows
def test_rows_reads_row_strided_views_in_place_and_copies_the_rest():
    base = torch.arange(15, dtype=torch.float32).view(3, 5)

    def check(t, in_place, ld):
        got, got_ld = _lib.rows(t)
        assert torch.equal(got, t) and got_ld == ld and isinstance(got_ld, int)
        assert (got.data_ptr() == t.data_ptr()) == in_place
        K, T = t.shape
        assert T <= 1 or got.stride(1) == 1
        if K > 1:                                                    # row k starts ld elements after row k - 1
            assert got.stride(0) == ld >= T
        assert torch.equal(got.as_strided((K, T), (ld, 1)), t)     # what a kernel reads from (pointer, ld)
        return got

    check(base, True, 5)                                             # contiguous
    wide = torch.arange(24, dtype=torch.float32).view(3, 8)
    window = wide[:, 2:7]
    assert window.shape == (3, 5) and not window.is_contiguous()
    check(window, True, 8)                                           # a column window: read in place
    assert check(base.t().contiguous().t(), False, 5).is_contiguous()                    # transposed: copied
    assert check(base[:1].expand(3, 5), False, 5).is_contiguous()    # stride(0) == 0: rows overlap, copied
    check(wide[1:2, 2:7], True, 5)                                   # one row of a wider tensor: ld = T
    check(base.t()[1:2], False, 3)                                   # one row, not unit stride: copied, ld = T
    col = wide[:, 3:4]
    assert col.shape == (3, 1) and col.stride() == (8, 1)
    check(col, True, 8)
    odd = wide.as_strided((3, 1), (8, 5), 3)                         # T = 1: stride(1) is never stepped
    check(odd, True, 8)
