"""CPU: the ragged batch of include/rfd_mesh_eval.h (rules B1 - B7) before any GPU run.  tests/objgrid_ref.py walks the
lattice as the kernels do (per-axis candidates, 32 x 32 bins, parity words per column); here it is held, word for word,
to the oracle tests/mesh_iou_f64.voxelize, which asks about every lattice point against every triangle.  That proves the
filter and the parity words.  The margins say how far every comparison of C3 / C4 / C5 is from equality: the equality of
the batched and the per-object path (tests/test_gpu_objgrid.py) rests on them."""
import numpy as np
import pytest
import torch

import mesh_iou_f64 as M
import objgrid_cases as C
import objgrid_ref as G

CASES = [(n, vs) for vs in C.FEW_SIZES for n in C.FEW] + [(n, vs) for vs in C.MANY_SIZES for n in C.MANY]
# an ulp of a lattice coordinate moves the quantities that are compared by about 1e-13 of their size
MARGIN = 1e-10


@pytest.mark.parametrize("name,voxel_size", CASES)
def test_restatement_equals_the_oracle(name, voxel_size):
    want, got = C.oracle(name, voxel_size), C.restated(name, voxel_size)
    if want.U is None:
        assert got.D == 0 and got.cnt == (0, 0) and name in ("empty", "nan", "empty_last")
        return
    assert got.D == want.S.shape[0] and (got.lo == want.lo).all() and got.cell == want.cell
    np.testing.assert_array_equal(got.S, M.pack_words(want.S))
    np.testing.assert_array_equal(got.I, M.pack_words(want.I))
    np.testing.assert_array_equal(got.U, M.pack_words(want.U))
    assert got.cnt == (int(want.U.sum()), int(want.S.sum())) and want.S.any()
    if name in ("doubled", "flat", "patch"):
        assert not want.I.any()
    elif voxel_size < 0.5:
        assert want.I.any()


def test_the_cube_crosses_the_word_boundaries():
    dims = [C.restated("cube", vs).D for vs in C.FEW_SIZES]
    assert dims == [2, 7, 63, 64, 65, 129]
    tetra = [C.restated("tetrahedron", vs).D for vs in C.FEW_SIZES]
    assert tetra[0] == 2 and tetra[-1] == 103
    many = [C.restated(n, vs).D for vs in C.MANY_SIZES for n in C.MANY]
    assert min(many) == 16 and max(many) == 31


def test_bins_hold_many_triangles_and_triangles_span_many_bins():
    unit = lambda n, vs: M.unit_vertices(C.OBJECTS[n][0], *M.frame(C.OBJECTS[n][0], 1, vs)[:2])
    v, f = C.OBJECTS["icosphere3"]
    st = G.constants(unit("icosphere3", C.MANY_SIZES[0])[f])
    lists, pairs = G.bin_lists(st[0] * unit("icosphere3", C.MANY_SIZES[0])[f] + st[1])
    assert max(len(m) for m in lists.values()) >= 16 and pairs > 4 * len(f)
    v, f = C.OBJECTS["cube"]
    st = G.constants(unit("cube", 0.5)[f])
    lists, pairs = G.bin_lists(st[0] * unit("cube", 0.5)[f] + st[1])
    assert len(lists) == G.BINS ** 2 and pairs >= 4 * G.BINS ** 2       # top and bottom: two triangles each, everywhere


@pytest.mark.parametrize("name,voxel_size", [c for c in CASES if c[0] not in ("empty", "nan", "empty_last", "flat")])
def test_margins(name, voxel_size):
    """The torus' lattice centres fall exactly on triangle edges: margin 0, it tests the strict inequalities of C4.  So
    do those of the patch, a regular grid of squares cut along x = y, whose diagonals the centres i == j lie on (0 at
    D = 16 and D = 26, float32 vertices or not).  No ulp can change the patch's words all the same: it is one open
    sheet, no column meets it twice, so P0 and P1 are never odd together.  Every other scene keeps its distance."""
    r = C.restated(name, voxel_size)
    print("%s at D = %d: margin %.3g over %d (bin, triangle) pairs" % (name, r.D, r.margin, r.pairs))
    if name == "torus":
        assert r.margin == 0.0
    elif name == "patch":
        assert r.margin == 0.0
        v, f = C.OBJECTS[name]
        lo, L, _, D = M.frame(v, len(f), voxel_size)
        n0, n1, _, _ = G.parities(M.unit_vertices(v, lo, L), f, D)
        assert (n0 + n1).max() == 1 and not (r.P0 & r.P1).any()
    else:
        assert r.margin >= MARGIN


def test_flat_object_has_no_constants():
    r = C.restated("flat", C.FEW_SIZES[1])
    assert r.D > 0 and r.pairs == 0 and not r.I.any() and r.S.any() and r.margin == np.inf


def test_restated_batch_layout():
    b = G.restate_batch(C.objects(C.FEW), C.FEW_SIZES[3])
    want = C.oracle_batch(C.FEW, C.FEW_SIZES[3])
    C.assert_same_grids(b, want)
    D = b["dims"].astype(np.int64)
    assert b["off"].tolist() == [0 if d == 0 else int((D[:k] ** 2 * ((D[:k] + 63) // 64)).sum()) for k, d in enumerate(D)]
    assert len(G.restate_batch([(C.NO_V, C.NO_F)])["words"]) == 1


def test_unknown_method_raises():
    from rfdnet_amd.iscnet import mesh_eval
    mesh = C.scene_mesh(C.objects(["tetrahedron"]), "cpu")
    with pytest.raises(ValueError, match="method"):
        mesh_eval.voxelize_objects(mesh, 0.5, method='nope')


@pytest.mark.parametrize("method", ["batched", "per_object"])
def test_cpu_tensors_are_refused(method):
    from rfdnet_amd.iscnet import mesh_eval
    mesh = C.scene_mesh(C.objects(["tetrahedron"]), "cpu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        mesh_eval.voxelize_objects(mesh, 0.5, method=method)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        mesh_eval.voxelize_objects(mesh, 0.5)
    assert isinstance(mesh.vertices, torch.Tensor)
