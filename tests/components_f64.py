"""Connected components of a mesh batch restated in numpy float64 / Python int (no test in here;
tests/test_components_cpu.py and tests/test_gpu_components.py import it).  It follows the six rules of
include/rfd_components.h literally -- a sequential union-find, one mesh, one component at a time -- and shares no code
with the package.  Every floating-point expression is written with the grouping of the rules, so an IEEE machine that
evaluates them as written (no fused multiply-add) computes the same sums up to the last place of each face's square
root."""
import numpy as np

LANES = 16
MEASURES = ('faces', 'area', 'abs_volume')


def valid_faces(f, nv):
    """rule 1 for the faces f (m,3) int64 of one mesh of nv vertices -> (m,) bool"""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < nv)).all(1) if len(f) else np.zeros(0, bool)


def label_mesh(f, nv):
    """rules 1 to 3 for one mesh -> (label (m,) int64, -1 for an invalid face; n components; vertex label (nv,) int64, -1
    for a vertex no valid face names)"""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ok = valid_faces(f, nv)
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]           # path halving: a parent stays an ancestor, the root stays the root
            x = parent[x]
        return x

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)           # the root of a set is its smallest index
    rows = f.tolist()
    for j, (a, b, c) in enumerate(rows):
        if ok[j]:
            union(a, b)
            union(a, c)
    named = np.zeros(nv, bool)
    named[f[ok].reshape(-1)] = True
    roots = sorted({find(i) for i in np.nonzero(named)[0].tolist()})       # ascending smallest index: rule 3
    number = {r: n for n, r in enumerate(roots)}
    label = np.array([number[find(row[0])] if ok[j] else -1 for j, row in enumerate(rows)], np.int64).reshape(-1)
    vlabel = np.array([number[find(i)] if named[i] else -1 for i in range(nv)], np.int64).reshape(-1)
    return label, len(roots), vlabel


def label(f, vend, tend):
    """-> dict: 'local', 'global' (F,) int64, 'n' (K ints), 'cbase' (K + 1 ints), 'vlabel' (V,) int64 global or -1"""
    vend, tend = [int(a) for a in vend], [int(a) for a in tend]
    f = np.asarray(f, np.int64).reshape(-1, 3)
    K = len(vend) - 1
    local, glob, vl, n, cbase = [], [], [], [], [0]
    for k in range(K):
        lab, nk, vlab = label_mesh(f[tend[k]:tend[k + 1]], vend[k + 1] - vend[k])
        local.append(lab)
        glob.append(np.where(lab >= 0, lab + cbase[-1], -1))
        vl.append(np.where(vlab >= 0, vlab + cbase[-1], -1))
        n.append(nk)
        cbase.append(cbase[-1] + nk)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return {'local': cat(local), 'global': cat(glob), 'n': n, 'cbase': cbase, 'vlabel': cat(vl)}


def tree_sum(terms):
    """the fixed summation shape: 16 partial sums (partial j: terms j, j + 16, ... in order, from 0), then 8, 4, 2, 1"""
    terms = np.asarray(terms, np.float64).reshape(-1)
    part = np.zeros(LANES)
    with np.errstate(all='ignore'):
        for at in range(0, len(terms), LANES):
            chunk = terms[at:at + LANES]
            part[:len(chunk)] = part[:len(chunk)] + chunk
        step = LANES // 2
        while step >= 1:
            part[:step] = part[:step] + part[step:2 * step]
            step //= 2
    return part[0]


def face_terms(p0, p1, p2):
    """rule 4 for faces with corners p0, p1, p2 (m,3) f64 -> a (m,), t (m,)"""
    with np.errstate(all='ignore'):
        u, v = p1 - p0, p2 - p0
        nx, ny, nz = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], \
            u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        L = np.sqrt((nx * nx + ny * ny) + nz * nz)
        a = np.where((L != 0) & np.isfinite(L), 0.5 * L, 0.0)
        cx, cy, cz = p1[:, 1] * p2[:, 2] - p1[:, 2] * p2[:, 1], p1[:, 2] * p2[:, 0] - p1[:, 0] * p2[:, 2], \
            p1[:, 0] * p2[:, 1] - p1[:, 1] * p2[:, 0]
        t = (p0[:, 0] * cx + p0[:, 1] * cy) + p0[:, 2] * cz
        t = np.where(np.isfinite(t), t, 0.0)
    return a, t


def measures(v, f, vend, tend, lab=None):
    """rule 4 -> dict over the C components: 'mesh', 'faces', 'vertices' int64, 'area', 'volume' f64, 'lo', 'hi' (C,3)"""
    lab = label(f, vend, tend) if lab is None else lab
    x = np.asarray(v).astype(np.float64).reshape(-1, 3)                  # f32 -> f64 is exact
    f = np.asarray(f, np.int64).reshape(-1, 3)
    vend, tend = [int(a) for a in vend], [int(a) for a in tend]
    C, K = lab['cbase'][-1], len(vend) - 1
    out = {'mesh': np.zeros(C, np.int64), 'faces': np.zeros(C, np.int64), 'vertices': np.zeros(C, np.int64),
           'area': np.zeros(C), 'volume': np.zeros(C), 'lo': np.full((C, 3), np.inf), 'hi': np.full((C, 3), -np.inf)}
    for k in range(K):
        xk, fk = x[vend[k]:vend[k + 1]], f[tend[k]:tend[k + 1]]
        lk = lab['local'][tend[k]:tend[k + 1]]
        for n in range(lab['n'][k]):
            c = lab['cbase'][k] + n
            rows = fk[lk == n]                                           # ascending face index
            p0, p1, p2 = xk[rows[:, 0]], xk[rows[:, 1]], xk[rows[:, 2]]
            a, t = face_terms(p0, p1, p2)
            with np.errstate(all='ignore'):
                out['area'][c], out['volume'][c] = tree_sum(a), tree_sum(t) / 6.0
            corners = np.concatenate([p0, p1, p2])
            for axis in range(3):
                col = corners[:, axis]
                col = col[np.isfinite(col)]
                if len(col):
                    out['lo'][c, axis], out['hi'][c, axis] = col.min(), col.max()
            out['mesh'][c], out['faces'][c] = k, len(rows)
            out['vertices'][c] = int((lab['vlabel'][vend[k]:vend[k + 1]] == c).sum())
    return out


def select(m, lab, keep='largest', measure='area', drop_cavities=False):
    """rule 5 -> keep_comp (C,) bool"""
    if measure not in MEASURES:
        raise ValueError("measure")
    largest_only = isinstance(keep, str)
    if largest_only and keep != 'largest':
        raise ValueError("keep")
    if not largest_only and not (0.0 <= float(keep) <= 1.0):
        raise ValueError("keep")
    val = {'faces': m['faces'].astype(np.float64), 'area': m['area'], 'abs_volume': np.abs(m['volume'])}[measure]
    out = np.zeros(lab['cbase'][-1], bool)
    for k in range(len(lab['n'])):
        c0, c1 = lab['cbase'][k], lab['cbase'][k + 1]
        if c1 == c0:
            continue
        best = c0
        for c in range(c0 + 1, c1):
            if val[c] > val[best]:
                best = c
        with np.errstate(all='ignore'):
            bar = (1.0 if largest_only else np.float64(keep)) * val[best]
            for c in range(c0, c1):
                stays = c == best or (not largest_only and val[c] >= bar)
                if stays and drop_cavities and c != best and m['volume'][c] * m['volume'][best] < 0:
                    stays = False
                out[c] = stays
    return out


def keep_components(v, f, vend, tend, keep='largest', measure='area', drop_cavities=False, pre=None):
    """rules 1 to 6 -> dict: 'v' (V2,3) in v's dtype, 'f' (F2,3) int64 local, 'vend', 'tend', 'found', 'kept' (lists),
    'rows' (V2,) int64: the input row every output vertex came from.  pre: (label(), measures()) of this batch, if the
    caller has them already"""
    v = np.asarray(v).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    vend, tend = [int(a) for a in vend], [int(a) for a in tend]
    lab = label(f, vend, tend) if pre is None else pre[0]
    keep_comp = select(measures(v, f, vend, tend, lab) if pre is None else pre[1], lab, keep, measure, drop_cavities)
    vend2, tend2, faces, rows, kept = [0], [0], [], [], []
    for k in range(len(vend) - 1):
        fk, gk = f[tend[k]:tend[k + 1]], lab['global'][tend[k]:tend[k + 1]]
        stays = np.array([g >= 0 and keep_comp[g] for g in gk], bool).reshape(-1)
        fk = fk[stays]
        used = np.zeros(vend[k + 1] - vend[k], bool)
        used[fk.reshape(-1)] = True
        renumber = np.cumsum(used) - 1
        faces.append(renumber[fk].reshape(-1, 3))
        rows.append(vend[k] + np.nonzero(used)[0])
        vend2.append(vend2[-1] + int(used.sum()))
        tend2.append(tend2[-1] + len(fk))
        kept.append(int(keep_comp[lab['cbase'][k]:lab['cbase'][k + 1]].sum()))
    rows = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    return {'v': v[rows], 'f': np.concatenate(faces).reshape(-1, 3) if faces else np.zeros((0, 3), np.int64),
            'vend': vend2, 'tend': tend2, 'found': list(lab['n']), 'kept': kept, 'rows': rows}
