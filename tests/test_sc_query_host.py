"""CPU checks of the Scan Context query entries (place recognition for scans outside the database): the C ABI declares,
binds and exports them; the chunk length of the candidate search is where the tests read it; the SLAM layer refuses a backend
that cannot run the query instead of falling back to something else."""
import os
import re

import numpy as np
import pytest

import randt_slam_amd as R
import sc_query_cases as sq
import scancontext_cases as cases
from oracle_backend import OracleBackend
from randt_slam_amd import _capi, slam, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("randt_sc_query_batch_dev", "randt_sc_db_query", "randt_sc_db_append_node")


def test_the_three_entries_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "randt.h")).read(), flags=re.S)
    lib = _capi.load()
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name + " is not declared in include/randt.h"
        assert name in _capi.SYMBOLS, name + " is not in _capi.SYMBOLS"
        assert hasattr(lib, name), name + " is not exported by the built library"
    # the declared argument counts are the bound ones
    for name in ENTRIES:
        args = re.search(r"\bint %s\s*\(([^;]*)\)\s*;" % name, hdr, flags=re.S).group(1)
        assert len(args.split(",")) == len(_capi.SYMBOLS[name][1]), name


def test_the_facade_declares_query_and_restore():
    hpp = open(os.path.join(ROOT, "include", "randt_facade.hpp")).read()
    assert "queryLoopClosure(" in hpp and "appendNode(" in hpp and "randt_sc_db_query(" in hpp and "randt_sc_db_append_node(" in hpp


def test_chunk_length_is_readable_and_the_cases_span_it():
    C = sq.chunk_length()
    c = cases.kernel_constants()
    assert C >= c["SC_BLOCK"] and C % c["SC_BLOCK"] == 0                   # whole strides of the workgroup
    p, db, qs, planted = sq.chunk_case()
    assert len(db["desc"]) == 3 * C + 17 and p["num_candidates"] < len(planted["tail"])
    # equal key distances inside a chunk, across every boundary and in the tail -- on the reference's own float distances
    _, d2 = sq.ref_candidates(p, db["rk"], qs["rk"][list(planted).index("boundary")])
    for b in (C, 2 * C, 3 * C):
        assert d2[b - 1] == d2[b] == 0
    _, d2 = sq.ref_candidates(p, db["rk"], qs["rk"][list(planted).index("tail")])
    assert (d2[planted["tail"]] == 0).all() and min(planted["tail"]) >= 3 * C and max(planted["tail"]) == len(d2) - 1
    _, d2 = sq.ref_candidates(p, db["rk"], qs["rk"][list(planted).index("inside")])
    assert (d2[planted["inside"]] == 0).all() and (np.diff(planted["inside"][1:]) == 1).all()
    want, _ = sq.ref_candidates(p, db["rk"], qs["rk"][list(planted).index("per_chunk")])
    assert [int(i) // C for i in want[:4]] == [0, 1, 2, 3]


def test_the_reference_decides_every_parity_case():
    """no shift tie and no sector-key tie in any candidate of any query of the independent pin (tests/test_gpu_sc_query.py),
    the best candidate well away from the next distinct one and from the threshold"""
    for name in sq.PARITY_SETS:
        p, db, qs = sq.parity_case(name, True)
        assert len(qs["desc"]) == sq.N_PARITY_QUERIES
        hits = 0
        for prior in (True, False):
            for j in range(len(qs["desc"])):
                r = sq.ref_query(p, db["desc"], db["rk"], db["pos"], db["dist"], qs["desc"][j], qs["rk"][j], qs["pos"][j] if prior else None,
                                 qs["dist"][j] if prior else None)
                assert not r["ties"], (name, j)
                d = np.unique(r["cand_dist"][r["cand_id"] >= 0])
                assert len(d) < 2 or d[1] - d[0] >= 1e-9, (name, j, d[:2])
                assert abs(r["min_dist"] - p["dist_thresh"]) >= 1e-9
                hits += r["loop"] >= 0
        assert hits >= 1, name
    assert cases.branches(cases.CONFIGS["staged_max"])["staged"] and not cases.branches(cases.CONFIGS["unstaged_min"])["staged"]
    assert len(sq.parity_case("indoor_600", True)[1]["desc"]) > sq.chunk_length()     # the shipped shape runs over two chunks


def test_relocalize_needs_a_backend_with_the_query():
    """the CPU oracle backend has no sc_query: NotImplementedError, not a quiet fall-back to something slower"""
    mp = R.default_matcher_params(parameterization=R.PARAM_MANIFOLD, gnc_steps=3)
    s = slam.Slam(OracleBackend(), mp, R.window_params(), R.default_matcher_params(gnc_steps=2), sc_params=dict(max_radius=20.0))
    scan = synth.make_scan(synth.make_world(), np.array([5.0, 0.0, np.pi / 2]), 1)
    with pytest.raises(NotImplementedError):
        s.relocalize(scan)
    assert not s.nodes and not s.edges
