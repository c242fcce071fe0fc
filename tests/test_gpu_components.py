"""GPU (-m gpu): connected components of a mesh batch on the device (rfdnet_amd/iscnet/components.py,
csrc/mesh_components.hip) against the numpy float64 restatement of its six rules (tests/components_f64.py).

Labels, counts, offsets, faces, volume, lo and hi must be EQUAL, and kept vertices bit-equal to the input rows they came
from.  `area` may differ by (faces + 1) * 2^-52 * area: both sides perform the same f64 operations in the same order, only
each face's square root may differ, in its last place.  The comparison prints the largest difference seen, in units of
2^-52 * area.

Measured on MI355X: the largest area difference of this file came out as 0 units (every area equal)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_cases as cases  # noqa: E402
import components_f64 as R  # noqa: E402
FRACTION = cases.FRACTION

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def dev(v, f, dtype=np.float64):
    """numpy batch -> device tensors (copies: the cases stay unchanged)"""
    return (torch.from_numpy(np.array(v, dtype=dtype).reshape(-1, 3)).cuda(),
            torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3)).cuda())


def labels_on_device(f, vend, tend):
    from rfdnet_amd.iscnet.components import label_components
    ft = torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3)).cuda()
    local, glob, n, cbase = label_components(ft, vend, tend)
    assert local.dtype == glob.dtype == torch.int32 and local.is_cuda and tuple(local.shape) == (len(f),)
    return local.cpu().numpy().astype(np.int64), glob.cpu().numpy().astype(np.int64), n, cbase


def keep_on_device(v, f, vend, tend, dtype=np.float64, **kw):
    from rfdnet_amd.iscnet.components import keep_components
    vt, ft = dev(v, f, dtype)
    v2, f2, vend2, tend2, info = keep_components(vt, ft, vend, tend, return_info=True, **kw)
    assert v2.dtype == vt.dtype and f2.dtype == torch.int32 and v2.is_cuda and f2.is_cuda
    assert tuple(v2.shape) == (vend2[-1], 3) and tuple(f2.shape) == (tend2[-1], 3)
    return v2.cpu().numpy(), f2.cpu().numpy().astype(np.int64), vend2, tend2, info


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_kept(name, got, want, v_in):
    v2, f2, vend2, tend2, info = got
    assert vend2 == want['vend'] and tend2 == want['tend'], (name, vend2, want['vend'], tend2, want['tend'])
    assert info == {'found': want['found'], 'kept': want['kept']}, (name, info)
    assert np.array_equal(f2, want['f']), name
    assert v2.dtype == v_in.dtype and np.array_equal(bits(v2), bits(v_in[want['rows']])), name


@pytest.fixture(scope="module")
def small():
    """the ragged batch of all the small cases with what the restatement makes of it, f64 and f32"""
    v, f, vend, tend = cases.batch(cases.small_meshes())
    lab = R.label(f, vend, tend)
    out = {'batch': (v, f, vend, tend), 'lab': lab}
    for dtype in (np.float64, np.float32):
        out[dtype] = R.measures(v.astype(dtype), f, vend, tend, lab)
    return out


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_ragged_batch_equals_the_restatement(hip, small, dtype):
    from rfdnet_amd.iscnet.components import component_measures, label_components
    v, f, vend, tend = small['batch']
    lab, want = small['lab'], small[dtype]
    vt, ft = dev(v, f, dtype)
    labels = label_components(ft, vend, tend)
    local, glob, n, cbase = labels
    assert np.array_equal(local.cpu().numpy(), lab['local']) and np.array_equal(glob.cpu().numpy(), lab['global'])
    assert n == lab['n'] and cbase == lab['cbase']
    worst = 0.0
    for given in (None, labels):                                            # labelled inside, and from the labels handed in
        got = {k: t.cpu().numpy() for k, t in component_measures(vt, ft, vend, tend, labels=given).items()}
        hip.device_status()
        for key in ('mesh', 'faces', 'vertices'):
            assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), key
        for key in ('volume', 'lo', 'hi'):
            assert got[key].dtype == np.float64 and np.array_equal(got[key], want[key]), key
        units = np.abs(got['area'] - want['area']) / np.where(want['area'] > 0, EPS * want['area'], 1.0)
        worst = max(worst, float(units.max()))
        print("ragged batch, %s: %d components, largest area difference %.3g units of 2^-52 area (allowed: faces + 1)"
              % (np.dtype(dtype).name, len(units), units.max()))
        assert (units <= want['faces'] + 1).all()
    assert want['faces'].tolist()[6:11] == list(cases.FAN_SIZES)            # the fans are where they are expected


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", cases.NUMBERINGS)
def test_a_long_strip_is_one_component_in_every_numbering(hip, how):
    v, f = cases.strip(how)
    local, glob, n, cbase = labels_on_device(f, [0, len(v)], [0, len(f)])
    hip.device_status()
    want = R.label(f, [0, len(v)], [0, len(f)])
    assert n == [1] == want['n'] and cbase == [0, 1]
    assert np.array_equal(local, want['local']) and np.array_equal(glob, want['global']) and (local == 0).all()


def test_the_cut_strip_and_permuted_face_rows(hip):
    v, f = cases.strip('random', 1000)
    want = R.label(f, [0, len(v)], [0, len(f)])
    local, glob, n, cbase = labels_on_device(f, [0, len(v)], [0, len(f)])
    assert n == [1000] == want['n'] and np.array_equal(local, want['local'])            # numbered by rule 3
    # two meshes in one batch: the natural strip with its face rows permuted, and the cut strip with its rows permuted
    s = cases.strip('natural')
    rng = np.random.default_rng(21)
    p, q = rng.permutation(len(s[1])), rng.permutation(len(f))
    bv, bf, vend, tend = cases.batch([(s[0], s[1][p]), (v, f[q])])
    local2, glob2, n2, cbase2 = labels_on_device(bf, vend, tend)
    hip.device_status()
    assert n2 == [1, 1000] and cbase2 == [0, 1, 1001]
    assert (local2[:len(p)] == 0).all() and np.array_equal(local2[len(p):], local[q])   # every face keeps its component
    assert np.array_equal(glob2[len(p):], local[q] + 1)


# 3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_keep_components_in_every_mode_and_measure(hip, small, dtype):
    v, f, vend, tend = small['batch']
    v_in = v.astype(dtype)
    pre = (small['lab'], small[dtype])
    for keep in ('largest', 0.0, FRACTION, 1.0):
        for measure in R.MEASURES:
            for drop in (False, True):
                name = "%s keep=%s measure=%s drop_cavities=%s" % (np.dtype(dtype).name, keep, measure, drop)
                want = R.keep_components(v_in, f, vend, tend, keep, measure, drop, pre=pre)
                got = keep_on_device(v, f, vend, tend, dtype, keep=keep, measure=measure, drop_cavities=drop)
                assert_kept(name, got, want, v_in)
    hip.device_status()
    tie = R.keep_components(v_in, f, vend, tend, 'largest', 'faces', pre=pre)
    assert tie['found'][4] == 3 and tie['kept'][4] == 1                      # the twins: the lower id of the tie stays
    assert tie['tend'][5] - tie['tend'][4] == 5


# 4 -------------------------------------------------------------------------------------------------------------------
def test_the_cavity(hip):
    from decimate_cases import sphere
    v, f = cases.cavity()
    vend, tend = [0, len(v)], [0, len(f)]
    v2, f2, vend2, tend2, info = keep_on_device(v, f, vend, tend, keep=0.0, drop_cavities=True)
    s = sphere()
    assert info == {'found': [2], 'kept': [1]} and vend2 == [0, len(s[0])] and tend2 == [0, len(s[1])]
    assert np.array_equal(f2, s[1]) and np.array_equal(bits(v2), bits(np.ascontiguousarray(s[0])))
    v3, f3, vend3, tend3, info3 = keep_on_device(v, f, vend, tend, keep=0.0)
    hip.device_status()
    assert info3 == {'found': [2], 'kept': [2]} and vend3 == vend and tend3 == tend
    assert np.array_equal(f3, f) and np.array_equal(bits(v3), bits(np.ascontiguousarray(v)))


# 5 -------------------------------------------------------------------------------------------------------------------
def test_a_mesh_alone_equals_itself_in_the_batch(hip, small):
    v, f, vend, tend = small['batch']
    whole = keep_on_device(v, f, vend, tend, keep=FRACTION, measure='area', drop_cavities=True)
    for k, (mv, mf) in enumerate(cases.small_meshes()):
        alone = keep_on_device(mv, mf, [0, len(mv)], [0, len(mf)], keep=FRACTION, measure='area', drop_cavities=True)
        vs, fs = slice(whole[2][k], whole[2][k + 1]), slice(whole[3][k], whole[3][k + 1])
        assert np.array_equal(bits(whole[0][vs]), bits(alone[0])) and np.array_equal(whole[1][fs], alone[1]), k
        assert alone[4] == {'found': [whole[4]['found'][k]], 'kept': [whole[4]['kept'][k]]}
    hip.device_status()


# 6 -------------------------------------------------------------------------------------------------------------------
def two_ball_grids(n=16):
    """K = 2 logit grids, each a large and a small ball well apart -> (both, the large ones alone) (2,n,n,n) f32"""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing='ij'), -1)
    ball = lambda c, r: r - np.sqrt(((g - np.asarray(c)) ** 2).sum(-1))
    large = np.stack([ball((5.2, 7.4, 7.6), 3.7), ball((9.9, 8.3, 7.1), 4.1)])
    small = np.stack([ball((12.6, 8.1, 7.9), 1.6), ball((2.4, 3.2, 7.7), 1.3)])
    return (torch.from_numpy(np.maximum(large, small).astype(np.float32)).cuda(),
            torch.from_numpy(large.astype(np.float32)).cuda())


def test_the_generator_drops_floaters_before_it_thins(hip, golden_dir):
    from rfdnet_amd.iscnet.components import label_components
    from rfdnet_amd.iscnet.decimate import decimate_meshes
    from seeded import seeded_onet
    fx = np.load(os.path.join(golden_dir, "F_GEN.npz"))
    both, large = two_ball_grids()

    def extract(grids, configure):
        g = configure(seeded_onet(fx, generation={'resolution_0': 8, 'upsampling_steps': 1}).generator)
        with torch.no_grad():
            meshes = g.extract_meshes(grids)
        hip.device_status()
        return g, meshes

    def same(a, b):
        assert a[0].dtype == b[0].dtype and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert list(a[2]) == list(b[2]) and list(a[3]) == list(b[3])

    plain, _ = extract(both, lambda g: g)
    clean, _ = extract(large, lambda g: g)
    assert plain.last_components is None
    assert plain.last_buffers[3][-1] > clean.last_buffers[3][-1] > 0
    kept, meshes = extract(both, lambda g: g.set_components('largest'))
    same(kept.last_buffers, clean.last_buffers)
    assert kept.last_components == {'found': [2, 2], 'kept': [1, 1]}
    assert len(meshes) == 2
    for m in meshes:
        nv, nf = m.vertices.shape[0], m.faces.shape[0]
        assert label_components(m.faces, [0, nv], [0, nf])[2] == [1]
    # with the decimation also set: the decimation of the filtered batch
    thin, _ = extract(both, lambda g: g.set_components('largest').set_decimation(8))
    v, f, vend, tend = clean.last_buffers
    want = decimate_meshes(v, f, vend, tend, 8, lo=np.full((2, 3), -0.55), h=np.full(2, 1.1 / 8))
    same(thin.last_buffers, want)
    assert 0 < want[3][-1] < tend[-1]
    # switched off again: what a generator that never heard of it makes
    off, _ = extract(both, lambda g: g.set_components('largest').set_components(None))
    same(off.last_buffers, plain.last_buffers)
    assert off.last_components is None


# 7 -------------------------------------------------------------------------------------------------------------------
def test_a_cpu_tensor_is_refused_and_so_is_a_null_pointer(hip):
    from rfdnet_amd.iscnet import components as C
    v, f = torch.zeros(3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int32)
    for call in (lambda: C.keep_components(v, f, [0, 3], [0, 1]), lambda: C.label_components(f, [0, 3], [0, 1]),
                 lambda: C.component_measures(v, f, [0, 3], [0, 1]),
                 lambda: C.keep_components(v.cuda(), f, [0, 3], [0, 1])):
        with pytest.raises(RuntimeError, match="CPU not supported"):
            call()
    # the launchers' own argument checks (nothing is launched)
    d = torch.device("cuda", 0)
    p = torch.zeros(16, dtype=torch.float64, device=d).data_ptr()
    with pytest.raises(hip.RfdHipError, match="null"):
        hip.call("rfd_components_union", d, 1, 1, 3, p, p, p, None)
    with pytest.raises(hip.RfdHipError, match="null"):
        hip.call("rfd_components_gather_vertices", d, 1, 1, 0, p, p, None, p)
    with pytest.raises(hip.RfdHipError, match="3 F"):
        hip.call("rfd_components_union", d, 2 ** 30, 1, 3, p, p, p, p)
    with pytest.raises(hip.RfdHipError, match="measure"):
        hip.call("rfd_components_select", d, 1, 1, 7, 1, 1.0, 0, p, p, p, p, p, p)
    with pytest.raises(hip.RfdHipError, match="fraction"):
        hip.call("rfd_components_select", d, 1, 1, 0, 0, 1.5, 0, p, p, p, p, p, p)
    # empty batches come back empty
    e = C.keep_components(v.cuda()[:0], f.cuda()[:0], [0, 0, 0], [0, 0, 0], return_info=True)
    assert e[0].shape == (0, 3) and e[0].dtype == torch.float64 and e[2] == [0, 0, 0] and e[4] == {'found': [0, 0], 'kept': [0, 0]}
    loose = C.keep_components(v.cuda(), f.cuda()[:0], [0, 3], [0, 0])
    assert loose[0].shape == (0, 3) and loose[2] == [0, 0] and loose[3] == [0, 0]
    hip.device_status()
