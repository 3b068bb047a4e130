"""Map::calculateCSDivergence (ndt_map.cpp:36-99) from its definition in numpy float64, and the random cells the CS tests feed
it.  No oracle, no HIP library: test_gpu_independent.py and test_gpu_csdiv_shapes.py both import this.

pair term   0.5 / sqrt(pi^2 det(Sa + Sb)) exp(-d^T (Sa + Sb)^-1 d / 2)
own term    over the cells with det(S) >= 1e-5: sqrt(det(S^-1)) / (2 pi) + twice the pair terms with every EARLIER cell
interaction over the fixed cells with det(S) >= 1e-5 x ALL moving cells
CS          -log I + log(F) / 2 + log(M) / 2"""
import numpy as np

GATE = 1e-5


def full(cov):
    """[n, 6] upper triangles (xx xy xi yy yi ii) -> [n, 3, 3] float64."""
    c = np.asarray(cov, dtype=np.float64).reshape(-1, 6)
    return c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def pair_terms(a, b):
    """[len(a), len(b)] pair terms of two cell arrays."""
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)))
    S = full(a["cov"])[:, None] + full(b["cov"])[None, :]
    d = a["mean"].astype(np.float64)[:, None, :] - b["mean"].astype(np.float64)[None, :, :]
    e = np.einsum("abi,abi->ab", d, np.linalg.solve(S, d[..., None])[..., 0])
    return 0.5 / np.sqrt(np.pi ** 2 * np.linalg.det(S)) * np.exp(-0.5 * e)


def valid_cells(cells, margin=0.05):
    """det(S) >= 1e-5 per cell.  Asserts that no cell sits within `margin` of the gate, where fp32 and fp64 could disagree."""
    det = np.linalg.det(full(cells["cov"])) if len(cells) else np.zeros(0)
    assert np.all(np.abs(det / GATE - 1.0) > margin)
    return det >= GATE


def own_term(cells):
    v = valid_cells(cells)
    if not v.any():
        return 0.0
    S = full(cells["cov"])[v]
    diag = np.sqrt(np.linalg.det(np.linalg.inv(S))) / (2 * np.pi)
    lower = np.tril(pair_terms(cells, cells), -1)[v]          # a valid cell against every earlier cell, valid or not
    return float(diag.sum() + 2.0 * lower.sum())


def cs_definition(fc, mc):
    """(divergence, [interaction, fixed term, moving term]) in float64."""
    inter = float(pair_terms(fc[valid_cells(fc)], mc).sum())
    terms = np.array([inter, own_term(fc), own_term(mc)])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(-np.log(terms[0]) + 0.5 * np.log(terms[1]) + 0.5 * np.log(terms[2])), terms


def rand_cells(rng, n, dtype, centres=None):
    """The recipe of test_cs_divergence_vs_numpy_definition, vectorised: random SPD covariances, every 7th cell scaled under
    the det(S) < 1e-5 gate, `centres` (means of another map) to cluster on so that the interaction term is not negligible.
    One addition to that recipe (whose scalar original stays in test_gpu_independent.py, with its own cells): cells within
    10 % of the gate are drawn again, so that the gate never depends on the precision of the determinant."""
    c = np.zeros(n, dtype=dtype)
    todo = np.arange(n)
    while len(todo):
        m = len(todo)
        if centres is None or len(centres) == 0:
            base = np.stack([rng.uniform(-8, 8, m), rng.uniform(-8, 8, m), rng.uniform(20, 80, m)], 1)
        else:
            base = np.asarray(centres, dtype=np.float64)[todo % len(centres)] + \
                np.stack([rng.uniform(-.3, .3, m), rng.uniform(-.3, .3, m), rng.uniform(-3, 3, m)], 1)
        A = rng.normal(0, 1, (m, 3, 3)) * [0.15, 0.15, 2.0]
        small = todo % 7 == 0
        S = A @ A.transpose(0, 2, 1) + np.where(small[:, None, None], np.diag([1e-5, 1e-5, 1e-4]), np.diag([1e-3, 1e-3, 1e-2]))
        S[small] *= 1e-2                                     # a few nearly degenerate cells: the det(S) < 1e-5 gate
        c["mean"][todo] = base
        c["cov"][todo] = S.reshape(m, 9)[:, [0, 1, 2, 4, 5, 8]]
        c["n"][todo] = 9
        det = np.linalg.det(full(c["cov"][todo]))            # of the float32 values the kernels will read
        todo = todo[np.abs(det / GATE - 1.0) <= 0.10]
    assert n == 0 or np.all(~valid_cells(c)[::7])
    return c
