"""CPU: rfdnet_amd/mesh_batch.py, the host side of a flat mesh batch: the vertex -> corner rows that the refinement, the
clustering decimation (cells as rows) and the edge collapse (dead faces -1 -1 -1) walk on the device.  No kernel runs here."""
import numpy as np
import torch

from rfdnet_amd.mesh_batch import corner_csr


def test_corner_csr():
    # vertex 2 twice in face 1, vertex 4 unreferenced, vertex 5 only in the last face
    faces = torch.tensor([[0, 1, 2], [2, 3, 2], [1, 0, 3], [5, 0, 1]])
    rowptr, col = corner_csr(faces, 6)
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32
    assert rowptr.tolist() == [0, 3, 6, 9, 11, 11, 12]
    rows = [col[rowptr[v]:rowptr[v + 1]].tolist() for v in range(6)]
    assert rows == [[0, 7, 10], [1, 6, 11], [2, 3, 5], [4, 8], [], [9]]          # ascending (face, corner)
    flat = faces.reshape(-1)
    assert all(int(flat[c]) == v for v in range(6) for c in rows[v])
    # an empty mesh in the middle of a batch is an empty range of both buffers; no faces at all: empty rows
    rowptr, col = corner_csr(torch.zeros(0, 3, dtype=torch.int64), 4)
    assert rowptr.tolist() == [0, 0, 0, 0, 0] and col.numel() == 0
    # an index outside the vertex range is in no row
    rowptr, col = corner_csr(torch.tensor([[0, 9, 1], [1, -1, 0]]), 2)
    assert rowptr.tolist() == [0, 2, 4] and col[:4].tolist() == [0, 5, 2, 3]
    # a dead face of the edge collapse (-1 -1 -1, int32) is in no row either, wherever it stands
    face = torch.tensor([[-1, -1, -1], [2, 0, 1], [-1, -1, -1], [1, 0, 2]], dtype=torch.int32)
    rowptr, col = corner_csr(face, 3)
    assert rowptr.tolist() == [0, 2, 4, 6] and col[:6].tolist() == [4, 10, 5, 9, 3, 11]
    assert sorted(col[6:].tolist()) == [0, 1, 2, 6, 7, 8]


def test_corner_csr_equals_the_counting_construction():
    """rowptr as the prefix sum of a bincount (which waits for the device to size its output) and as a search in the
    sorted keys are the same rows, for indices on both sides of [0, n) and for one row"""
    rng = np.random.default_rng(3)
    for n, F in ((1, 5), (7, 0), (7, 40), (50, 33)):
        faces = torch.from_numpy(rng.integers(-3, n + 3, size=(F, 3)))
        flat = faces.reshape(-1)
        flat = torch.where((flat >= 0) & (flat < n), flat, torch.full_like(flat, n))
        want = torch.zeros(n + 1, dtype=torch.int64)
        want[1:] = torch.cumsum(torch.bincount(flat, minlength=n + 1)[:n], 0)
        rowptr, col = corner_csr(faces, n)
        assert torch.equal(rowptr.long(), want) and torch.equal(col.long(), torch.sort(flat, stable=True).indices)
