"""GPU (-m gpu): the ragged-batch voxeliser csrc/objgrid.hip behind mesh_eval.voxelize_objects(method='batched')
(include/rfd_mesh_eval.h, rules B1 - B7).

No tolerance anywhere: the result is bit words and integer counts, and they are held byte for byte to the oracle
tests/mesh_iou_f64.voxelize (numpy over tests/mesh_sample_ref.py), computed once per (object, voxel size) in
tests/objgrid_cases.py.  The per-object path is the cross-check, never the oracle."""
import contextlib

import numpy as np
import pytest
import torch

import mesh_iou_f64 as M
import mesh_sample_ref as R
import objgrid_cases as C

pytestmark = pytest.mark.gpu
NOT_TORUS = [n for n in C.MANY if n != "torus"]


def voxelize(names, voxel_size, **kw):
    from rfdnet_amd.iscnet import mesh_eval
    return mesh_eval.voxelize_objects(C.scene_mesh(C.objects(names), "cuda"), voxel_size, **kw)


def check_against_oracle(names, voxel_size):
    grids = voxelize(names, voxel_size)
    want = C.oracle_batch(names, voxel_size)
    got = C.grids_as_numpy(grids)
    print("D = %s, %d words, cnt %s" % (got["dims"].tolist(), len(got["words"]), got["cnt"].tolist()))
    C.assert_same_grids(got, want)
    assert grids.dims.tolist() == want["dims"].tolist() and len(grids) == len(names)
    for k, n in enumerate(names):                                            # ObjectGrids.grid: U unpacked on the device
        o, g = C.oracle(n, voxel_size), grids.grid(k)
        assert (g is None) == (o.U is None)
        if g is not None:
            assert g.dtype == torch.bool and g.is_cuda and np.array_equal(g.cpu().numpy(), o.U)
    return grids


# ------------------------------------------------------------------------------------------------ 1, 2: the oracle
@pytest.mark.parametrize("voxel_size", C.FEW_SIZES)
def test_few_face_scene_equals_the_oracle(hip, voxel_size):
    grids = check_against_oracle(C.FEW, voxel_size)
    dims = grids.dims.tolist()
    assert dims[0] == dims[3] == dims[8] == 0 and min(dims[1:3] + dims[4:8]) >= 2
    cnt = grids.cnt.cpu().numpy()
    assert cnt[4, 0] == cnt[4, 1] > 0 and cnt[7, 0] == cnt[7, 1] > 0         # doubled face, flat: S without I
    assert hip.stream_status_bits() == 0


@pytest.mark.parametrize("voxel_size", C.MANY_SIZES)
def test_many_face_scene_equals_the_oracle(hip, voxel_size):
    grids = check_against_oracle(C.MANY, voxel_size)
    assert 16 <= min(grids.dims) and max(grids.dims) <= 31
    assert hip.stream_status_bits() == 0


# ------------------------------------------------------------------------------------------------ 3: four words per row
def unpack(words, D):
    """(D * D * W,) uint64 -> (D,D,64 W) bool, every bit"""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder='little')
    return bits.reshape(D, D, -1).astype(bool)


@pytest.mark.parametrize("D", [193, 256])
def test_four_words_per_row(hip, D):
    """S against the per-object voxeliser (the surface rule has no lattice division), I against
    mesh_sample_ref.contains on the z slabs at the word boundaries and on 100 000 seeded lattice points"""
    from rfdnet_amd.iscnet import mesh_eval
    v, f = C.OBJECTS["tetrahedron"]
    lo, hi = v.min(0), v.max(0)
    L = (hi - lo).max()
    voxel_size = L / (D + 0.5)
    assert M.frame(v, len(f), voxel_size)[3] == D
    mesh = C.scene_mesh([(v, f)], "cuda")
    b = mesh_eval.batched_words(mesh, voxel_size)
    assert b.dims.tolist() == [D] and b.S.numel() == D * D * 4
    S = unpack(b.S.cpu().numpy().view(np.uint64), D)
    I = unpack(b.I.cpu().numpy().view(np.uint64), D)
    assert not S[:, :, D:].any() and not I[:, :, D:].any()                  # bits at z >= D are zero
    S_po = mesh_eval.object_grids(mesh, voxel_size)[0][0].cpu().numpy()
    assert np.array_equal(S[:, :, :D], S_po) and S_po.any()
    unit = M.unit_vertices(v, lo, L)
    c = (np.arange(D) + 0.5) / D - 0.5
    slabs = sorted(set([63, 64, 127, 128, 191, 192, D - 1]))
    ij = np.stack(np.meshgrid(np.arange(D), np.arange(D), indexing='ij'), -1).reshape(-1, 2)
    idx = np.concatenate([np.concatenate([ij, np.full((len(ij), 1), z)], 1) for z in slabs] +
                         [np.random.default_rng(7).integers(0, D, (100000, 3))])
    want = R.contains(unit, f, c[idx])[0]
    got = I[idx[:, 0], idx[:, 1], idx[:, 2]]
    print("D = %d: %d points, %d inside; |S| = %d, |I| = %d" % (D, len(idx), want.sum(), S.sum(), I.sum()))
    assert np.array_equal(got, want) and want.any() and not want.all()
    grids = mesh_eval.voxelize_objects(mesh, voxel_size)
    U = unpack(grids.words.cpu().numpy().view(np.uint64), D)
    assert np.array_equal(U, S | I) and grids.cnt.cpu().tolist() == [[int((S | I).sum()), int(S.sum())]]
    assert hip.stream_status_bits() == 0


# ------------------------------------------------------------------------------------------------ 4: the existing path
@pytest.mark.parametrize("names,voxel_size", [(C.FEW, vs) for vs in C.FEW_SIZES] + [(NOT_TORUS, vs) for vs in C.MANY_SIZES])
def test_equals_the_per_object_path(hip, names, voxel_size):
    """Holds with a margin only: the per-object path takes its lattice from torch's division of a tensor by a number,
    which may be a product with the reciprocal, an ulp away; tests/test_objgrid_cpu.py::test_margins holds these scenes
    to a margin of 1e-10 (the patch: to a single crossing per column)."""
    a, b = voxelize(names, voxel_size), voxelize(names, voxel_size, method='per_object')
    C.assert_same_grids(C.grids_as_numpy(a), C.grids_as_numpy(b))
    assert a.dims.tolist() == b.dims.tolist()


# ------------------------------------------------------------------------------------------------ 5: independence
def test_independence(hip):
    from rfdnet_amd.iscnet import mesh_eval
    for names, vs in ((C.FEW, C.FEW_SIZES[3]), (C.MANY, C.MANY_SIZES[0])):
        whole = C.grids_as_numpy(voxelize(names, vs))
        again = C.grids_as_numpy(voxelize(names, vs))
        C.assert_same_grids(again, whole)                                     # two calls are bitwise equal
        n_words = lambda D: int(D) * int(D) * ((int(D) + 63) // 64)
        rows = lambda g, k: (int(g["dims"][k]), g["frame"][k].tobytes(), tuple(g["cnt"][k]),
                             g["words"][g["off"][k]:g["off"][k] + n_words(g["dims"][k])].tobytes())
        for k, n in enumerate(names):                                         # every object alone
            alone = C.grids_as_numpy(voxelize([n], vs))
            assert rows(alone, 0) == rows(whole, k), n
        back = C.grids_as_numpy(voxelize(names[::-1], vs))                    # reverse order: the reversed rows
        for k in range(len(names)):
            assert rows(back, len(names) - 1 - k) == rows(whole, k)
    a, b = voxelize(C.FEW, C.FEW_SIZES[1]), voxelize(C.FEW, C.FEW_SIZES[1], method='per_object')
    (iou_a, cnt_a), (iou_b, cnt_b) = mesh_eval.mesh_iou(a, a), mesh_eval.mesh_iou(b, b)
    assert iou_a.cpu().numpy().tobytes() == iou_b.cpu().numpy().tobytes() and torch.equal(cnt_a, cnt_b)
    assert float(iou_a[1, 1]) == 1.0 and float(iou_a[0, 0]) == 0.0
    assert hip.stream_status_bits() == 0


# ------------------------------------------------------------------------------------------------ 6: refusals
@contextlib.contextmanager
def counted_launches(hip, monkeypatch, log):
    call = hip.call

    def counting(name, *a):
        log.append(name)
        return call(name, *a)
    with monkeypatch.context() as m:
        m.setattr(hip, "call", counting)
        yield


def test_refusals(hip, monkeypatch):
    from rfdnet_amd.iscnet import mesh_eval
    dev = torch.device("cuda")
    with pytest.raises(ValueError):
        voxelize(C.FEW, 1.0 / 300)                                            # D > 256
    # a cube face that indexes into the tetrahedron's vertices: refused from the read-back, nothing launched
    mesh = C.scene_mesh(C.objects(["cube", "tetrahedron"]), "cuda")
    mesh.faces[5, 1] = 9
    log = []
    with counted_launches(hip, monkeypatch, log):
        for method in ("batched", "per_object"):
            with pytest.raises(ValueError):
                mesh_eval.voxelize_objects(mesh, 0.25, method=method)
    assert log == []
    # the launchers: valid arguments of a one-object batch, then one of them made bad; sentinels in what they write
    F, N, n_words = 4, 1, 4
    tri32 = torch.zeros(F, 3, 3, device=dev)
    tri64 = torch.zeros(F, 3, 3, dtype=torch.float64, device=dev)
    fobj = torch.zeros(F, dtype=torch.int32, device=dev)
    dim, off = torch.full((1,), 2, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    consts = torch.ones(1, 6, dtype=torch.float64, device=dev)
    words, inter = (torch.full((n_words,), 5, dtype=torch.int64, device=dev) for _ in range(2))
    cursor = torch.full((1024,), 5, dtype=torch.int32, device=dev)
    offsets = torch.zeros(1025, dtype=torch.int32, device=dev)
    lst, cnt = torch.full((16,), 5, dtype=torch.int32, device=dev), torch.full((1, 2), 5, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()

    def host(d=2, o=0):
        return np.array([d], np.int32), np.array([o], np.int64)

    def surface(F=F, tri=p(tri32), N=N, d=2, o=0, n_words=n_words):
        dh, oh = host(d, o)
        hip.call("rfd_objgrid_surface", dev, F, tri, p(fobj), N, dh.ctypes.data, oh.ctypes.data, p(dim), p(off), n_words, p(words))

    def bins(F=F, tri=p(tri64), N=N, d=2, n_pairs=16):
        dh, _ = host(d)
        hip.call("rfd_objgrid_bins", dev, F, tri, p(fobj), N, dh.ctypes.data, p(dim), p(consts), p(cursor), p(lst), n_pairs)

    def interior(F=F, tri=p(tri64), N=N, d=2, o=0, n_words=n_words, n_pairs=16):
        dh, oh = host(d, o)
        hip.call("rfd_objgrid_interior", dev, F, tri, N, dh.ctypes.data, oh.ctypes.data, p(dim), p(off), n_words, p(consts),
                 p(offsets), p(lst), n_pairs, p(inter))

    def finish(N=N, d=2, o=0, n_words=n_words, w=p(words)):
        dh, oh = host(d, o)
        hip.call("rfd_objgrid_finish", dev, N, dh.ctypes.data, oh.ctypes.data, p(dim), p(off), n_words, w, p(inter), p(cnt))

    bad_table = [dict(d=1), dict(d=257), dict(d=-2), dict(o=1), dict(o=-1), dict(N=-1)]
    refused = [(surface, [dict(F=-1), dict(tri=None), dict(n_words=-1), dict(n_words=3)] + bad_table),
               (bins, [dict(F=-1), dict(tri=None), dict(n_pairs=-1), dict(d=1), dict(d=257), dict(d=-2), dict(N=-1)]),
               (interior, [dict(F=-1), dict(tri=None), dict(n_pairs=-1), dict(n_words=-1), dict(n_words=3)] + bad_table),
               (finish, [dict(w=None), dict(n_words=-1), dict(n_words=3)] + bad_table)]
    for fn, cases in refused:
        for kw in cases:
            with pytest.raises(hip.RfdHipError):
                fn(**kw)
    torch.cuda.synchronize()
    for t in (words, inter, cursor, lst, cnt):
        assert (t == 5).all()
    # afterwards the stream still computes scene 1
    check_against_oracle(C.FEW, C.FEW_SIZES[1])
    assert hip.stream_status_bits() == 0


# ------------------------------------------------------------------------------------------------ 7: structure
@contextlib.contextmanager
def counted_readbacks(counter):
    """tools/mesh_eval_cost.py's count: read-backs of a device tensor through .cpu() / .item() / int() / ..."""
    names = ('cpu', 'item', 'tolist', '__int__', '__float__', '__bool__', '__index__')
    saved = {n: getattr(torch.Tensor, n) for n in names}
    depth = [0]

    def wrap(fn):
        def counted(self, *a, **k):
            if self.is_cuda and depth[0] == 0:
                counter[0] += 1
            depth[0] += 1
            try:
                return fn(self, *a, **k)
            finally:
                depth[0] -= 1
        return counted
    for n in names:
        setattr(torch.Tensor, n, wrap(saved[n]))
    try:
        yield
    finally:
        for n in names:
            setattr(torch.Tensor, n, saved[n])


def test_read_backs_and_launches_do_not_grow_with_the_objects(hip, monkeypatch):
    from rfdnet_amd.iscnet import mesh_eval
    seen = []
    for copies in (4, 40):
        mesh = C.scene_mesh(C.objects(["tetrahedron"] * copies), "cuda")
        syncs, log = [0], []
        with counted_launches(hip, monkeypatch, log), counted_readbacks(syncs):
            grids = mesh_eval.voxelize_objects(mesh, C.FEW_SIZES[1])
        assert len(grids) == copies and grids.cnt.cpu()[:, 0].min() > 0
        seen.append((syncs[0], sorted(n for n in log if n.startswith("rfd_objgrid"))))
    print(seen)
    assert seen[0] == seen[1] and 0 < seen[0][0] <= 3
    assert seen[0][1] == ["rfd_objgrid_bins", "rfd_objgrid_bins", "rfd_objgrid_finish", "rfd_objgrid_interior",
                          "rfd_objgrid_surface"]
