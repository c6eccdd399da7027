"""CPU: the fp64 brute force of tests/knn_oracle.py (the checker of the GPU k-NN) agrees with the reference's own
method, sklearn NearestNeighbors(k + 1).kneighbors(x)[:, 1:] (sgn_splatfacto.py:439-457), duplicates included."""
import numpy as np
import pytest

import knn_oracle as KO

sk = pytest.importorskip("sklearn.neighbors")


def _sklearn(x, k):
    d, i = sk.NearestNeighbors(n_neighbors=k + 1, algorithm="auto", metric="euclidean").fit(x).kneighbors(x)
    return d[:, 1:], i[:, 1:]


@pytest.mark.parametrize("name", ["ragged", "repeat5", "lattice", "collinear", "tiny"])
@pytest.mark.parametrize("k", [1, 3, 16])
def test_brute_force_matches_sklearn_distances(name, k):
    x = KO.cloud(f"tiny{k}" if name == "tiny" else name)     # tiny: N = k + 1
    rows = np.arange(0, x.shape[0], max(1, x.shape[0] // 3000))
    d, i = KO.knn_brute(x, k, rows=rows)
    ds, _ = _sklearn(x, k)
    # (sklearn's kd-tree computes in float64; for a handful of points "auto" picks its brute force, which works in the
    # input's float32 — hence the float32-sized tolerance)
    np.testing.assert_allclose(d, ds[rows], rtol=1e-6, atol=1e-6)
    assert (i != rows[:, None]).all()
    xd = x.astype(np.float64)
    np.testing.assert_allclose(np.linalg.norm(xd[rows, None] - xd[i], axis=-1), d, rtol=1e-12, atol=0)


def test_sklearn_first_column_is_often_not_the_query_with_duplicates():
    """Why the contract is about the distance MULTISET: with each point repeated 5x, sklearn's dropped first column is
    frequently another copy, yet it is a 0 either way."""
    x = KO.cloud("repeat5")[:5000]
    d, i = sk.NearestNeighbors(n_neighbors=4).fit(x).kneighbors(x)
    assert (d[:, 0] == 0).all()
    assert (i[:, 0] != np.arange(x.shape[0])).sum() > 0
