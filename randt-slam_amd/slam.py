"""The reference's full SLAM loop as a call-pattern harness (row f-4): LocalFuser::processScan's graph bookkeeping
(src/local_fuser/local_fuser.cpp:164-223 keyframe node + odometry edge, :247-279 submap root node),
LocalFuser::detectLoopClosures (:318-416: the Scan Context branch, and -- loop_search="covariance" -- the branch gated by the
nodes' marginal covariances, :351-412, dead in the reference since its covariance block is commented out), NDTSlam::optimizePoseGraph (src/ndt_slam/ndt_slam.cpp:
351-361 -> GlobalFuser::optimizePoseGraph) and the pose part of LocalFuser::updateSubmaps (:65-88).

Everything numeric goes through the injected backend (odometry.HipBackend = the C ABI: NDT build, window registration,
Scan Context, pair registration, CS divergence, pose graph; tests inject an oracle backend with the same methods).  Not
built: OGM ray tracing / HierarchicalMap occupancy layers (SURVEY: out of scope), ROS timers (the caller decides when
to search and when to optimise)."""
import math

import numpy as np

from .odometry import Odometry, _se2_inv4, _se2_mul4

ODOM_SQRT_INFO = np.diag([10.0, 10.0, 50.0])          # local_fuser.cpp:203-205, :264-266


def _pose4(theta, x, y):
    return np.array([math.cos(theta), math.sin(theta), x, y])


def _angle(p4):
    return math.atan2(p4[1], p4[0])                    # so2().log()


def _mahalanobis2(cov, dx, dy):
    """sqrt(d^T cov_pos_pos^-1 d) with the closed-form 2x2 inverse, or None if cov_pos_pos is not positive definite."""
    a, b, c, d = cov[0, 0], cov[0, 1], cov[1, 0], cov[1, 1]
    det = a * d - b * c
    if not (a > 0.0 and det > 0.0):
        return None
    return math.sqrt((d * dx * dx - (b + c) * dx * dy + a * dy * dy) / det)


def _smaller_eigenvalue2(cov):
    """Smaller eigenvalue of the self-adjoint xy block (lower triangle read, like Eigen::SelfAdjointEigenSolver)."""
    a, c, d = cov[0, 0], cov[1, 0], cov[1, 1]
    return 0.5 * (a + d) - math.sqrt(0.25 * (a - d) * (a - d) + c * c)


class Slam(Odometry):
    keep_filtered_points = True

    def __init__(self, backend, matcher_params, window_params, loop_matcher_params, params=None, sc_params=None,
                 loop_closure_max_cs_divergence=3.6, loop_closure_weight=4.0e4, loop_sqrtI=None, pg_params=None,
                 loop_search="scan_context", max_data_association_mahalanobis_dist=0.5, compute_dfs_loop_closure=False,
                 bnb_params=None, bnb_matcher_params=None, loop_closure_scale=1.5, batch_loop_search=False):
        super().__init__(backend, matcher_params, window_params, params)
        if loop_search not in ("scan_context", "covariance"):
            raise ValueError("loop_search must be 'scan_context' or 'covariance'")
        self.loop_search = loop_search
        # covariance mode: the candidates of all pending queries as ONE device batch (a backend without loop_candidates_batch
        # runs them one by one)
        self.batch_loop_search = bool(batch_loop_search)
        self.loop_batches = []         # covariance mode: candidates per detect_loop_closures call
        self.max_mahalanobis = float(max_data_association_mahalanobis_dist)   # base yaml :26
        self.compute_dfs = bool(compute_dfs_loop_closure)                     # base yaml :25
        self.bnb_params = bnb_params                                          # csm_* of the matcher (backend default if None)
        self.bnb_mp = bnb_matcher_params if bnb_matcher_params is not None else loop_matcher_params
        self.loop_scale = float(loop_closure_scale)
        self.loop_mp = loop_matcher_params
        self.max_cs = loop_closure_max_cs_divergence   # parameters_indoor.yaml:8
        self.loop_sqrt_info = loop_closure_weight * (np.eye(3) if loop_sqrtI is None else np.asarray(loop_sqrtI, dtype=np.float64))
        self.pg_params = dict(pg_params or {})
        if loop_search == "scan_context":
            backend.sc_open(dict(sc_params or {}))
        self.nodes = []                # global pose4 per node id (std::map<int, Pose>, keys 0..n-1)
        self.traversed = []            # Pose::traversed_dist
        self.edges = []                # (id_begin, id_end, trans pose4, sqrt_information 3x3)
        self.submap_idzs = []          # node id -> submap index
        self.root_nodes = {}           # submap index -> node id
        self.node_scans = {}           # scans_: node id -> scan handle (kept alive)
        self.submaps = {}              # submaps_: finished submap index -> submap handle
        self.pending_loop_search = []  # _next_maps_to_search_loop
        self.loop_log = []             # (query node, candidate node, cs divergence, accepted)
        self.n_optimizations = 0
        self.node_cov = []             # covariance mode: Pose::cov per node (3x3, zeros until an optimisation covered the node)
        self.n_covariance_failures = 0

    # ---- graph bookkeeping ------------------------------------------------------------------
    def _add_node(self, pose4, scan, points):
        nid = len(self.nodes)
        if nid > 0:                                                                       # :199-205, :258-267
            trans = _se2_mul4(_se2_inv4(self.nodes[nid - 1]), pose4)
            self.edges.append((nid - 1, nid, trans, ODOM_SQRT_INFO))
            dist = self.traversed[nid - 1] + float(np.hypot(trans[2], trans[3]))
        else:
            dist = 0.0
        self.nodes.append(np.array(pose4, dtype=np.float64))
        self.traversed.append(dist)
        self.submap_idzs.append(self.n_finished_submaps)
        self.node_scans[nid] = scan
        self._ref(scan)
        self.node_cov.append(np.zeros((3, 3)))
        if self.loop_search == "scan_context":
            self.b.sc_append(points, pose4[2:], dist)                                     # :207, :281
        return nid

    def _on_first_scan(self, scan, points):
        nid = self._add_node(self.current_global_transform, scan, points)                 # :247-279
        self.root_nodes[self.n_finished_submaps] = nid

    def _on_keyframe(self, scan, points, smoothed_pose4):
        nid = self._add_node(_se2_mul4(self.current_global_transform, smoothed_pose4), scan, points)   # :192-222
        self.pending_loop_search.append(nid)

    def _on_submap_finished(self, submap):
        self.submaps[self.n_finished_submaps] = submap                                    # :43
        return True

    # ---- LocalFuser::detectLoopClosures, Scan Context branch (:318-350) ------------------------
    def _scan_context_candidate(self, q):
        """The candidate of query node q as (q, candidate node, submap, guess), or None."""
        lid, yaw = self.b.sc_detect(q)                                                                # :323
        if lid == -1 or self.submap_idzs[q] == self.submap_idzs[lid]:
            return None
        sub_i = self.submap_idzs[lid]
        if sub_i not in self.submaps:          # submaps_.at() would throw: the candidate's submap is still being built
            return None
        root = self.nodes[self.root_nodes[sub_i]]
        return q, lid, sub_i, _se2_mul4(_se2_mul4(_se2_inv4(root), self.nodes[lid]), _pose4(-yaw, 0.0, 0.0))   # :333

    def detect_loop_closures(self):
        if self.loop_search == "covariance":
            return self._detect_loop_closures_covariance()
        added = 0
        while self.pending_loop_search:
            cand = self._scan_context_candidate(self.pending_loop_search.pop(0))
            if cand is None:
                continue
            q, lid, sub_i, guess = cand
            est, _cost = self.b.register_pair(self.submaps[sub_i], self.node_scans[q], self.loop_mp, guess)   # :335
            cs = self.b.cs_divergence(self.submaps[sub_i], self.node_scans[q], est)                     # :338-339
            added += self._close_loop(q, lid, sub_i, est, cs)                                           # :340-347
        return added

    # ---- place recognition for a scan that is not part of the session (no counterpart in the reference) ----------
    def relocalize(self, points, max_candidates=None):
        """Where in the map was this scan taken?  For a restart, a tracking loss, or a scan of another session: the scan is
        queried against the WHOLE Scan Context database without an odometry prior (it has none), every candidate below
        dist_thresh whose submap is finished is refined exactly like a loop-closure candidate (:333-339: the same guess, the
        same registration against the submap, the same CS divergence), and the candidate with the smallest divergence below
        loop_closure_max_cs_divergence wins.  Neither the graph nor the database changes.
        points: (N, stride) scan as process_scan takes it; max_candidates: at most this many ranks are refined (None: all).
        Returns None, or a dict: pose (global pose4 of the scan), node (the candidate), submap, cs_divergence, sc_distance."""
        if not hasattr(self.b, "sc_query"):
            raise NotImplementedError("relocalize needs a backend with sc_query (odometry.HipBackend)")
        if self.loop_search != "scan_context":
            raise ValueError("relocalize needs loop_search='scan_context': there is no Scan Context database in this session")
        scan = self.b.build_scan(points)
        try:
            _, _, _, cand_id, cand_yaw, cand_dist = self.b.sc_query(points)
            n = len(cand_id) if max_candidates is None else min(len(cand_id), int(max_candidates))
            best = None
            for lid, yaw, dist in zip(cand_id[:n].tolist(), cand_yaw[:n].tolist(), cand_dist[:n].tolist()):
                if lid < 0 or not dist < self.b.sc_dist_thresh():
                    continue
                sub_i = self.submap_idzs[lid]
                if sub_i not in self.submaps:                  # the candidate's submap is still being built
                    continue
                root = self.nodes[self.root_nodes[sub_i]]
                guess = _se2_mul4(_se2_mul4(_se2_inv4(root), self.nodes[lid]), _pose4(-yaw, 0.0, 0.0))   # as _scan_context_candidate
                est, _cost = self.b.register_pair(self.submaps[sub_i], scan, self.loop_mp, guess)
                cs = float(self.b.cs_divergence(self.submaps[sub_i], scan, est))
                if cs < self.max_cs and (best is None or cs < best["cs_divergence"]):
                    best = dict(pose=_se2_mul4(root, est), node=lid, submap=sub_i, cs_divergence=cs, sc_distance=dist)
            return best
        finally:
            self.b.release_scan(scan)

    # ---- LocalFuser::detectLoopClosures, the branch without Scan Context (:351-412), quirks included -------
    def _covariance_candidates(self, q):
        """The candidates of query node q: per finished submap within the gate its closest node, in std::map order, as
        (q, candidate node, submap, guess, search windows or None)."""
        thr = self.max_mahalanobis
        best = {}                                  # submap -> (node, dist): the closest node of every finished submap
        tq = self.nodes[q]
        for i in range(len(self.nodes)):
            sub_i = self.submap_idzs[i]
            if sub_i == self.submap_idzs[q] or sub_i == self.n_finished_submaps or sub_i not in self.submaps:   # :355
                continue
            dist = _mahalanobis2(self.node_cov[i], tq[2] - self.nodes[i][2], tq[3] - self.nodes[i][3])           # :357, the NODE's covariance
            if dist is None:                       # never covered by an optimisation (the reference: NaN < thr is false)
                continue
            if dist < thr and (sub_i not in best or dist < best[sub_i][1]):                                     # :358-362
                best[sub_i] = (i, dist)
        out = []
        for sub_i in sorted(best):                 # std::map order
            lid = best[sub_i][0]
            root = self.nodes[self.root_nodes[sub_i]]
            guess = _se2_mul4(_se2_inv4(root), tq)                                                              # :376
            windows = None
            if self.compute_dfs:                                                                                # :379-388
                cov = self.node_cov[lid]
                lam0 = _smaller_eigenvalue2(cov)   # eigenvalues()(0): the SMALLER one, named "max" there, no root taken
                windows = (thr * abs(lam0), min(2 * math.pi, thr * math.sqrt(cov[2, 2])))
            out.append((q, lid, sub_i, guess, windows))
        return out

    def _close_loop(self, q, lid, sub_i, est, cs):
        ok = bool(cs < self.max_cs)
        self.loop_log.append((q, lid, float(cs), ok))
        if ok:
            self.edges.append((self.root_nodes[sub_i], q, np.array(est, dtype=np.float64), self.loop_sqrt_info))   # :341-347, :402-409
        return int(ok)

    def _detect_loop_closures_covariance(self):
        if self.batch_loop_search and hasattr(self.b, "loop_candidates_batch"):
            return self._detect_loop_closures_covariance_batched()
        added = n_cands = 0
        while self.pending_loop_search:
            q = self.pending_loop_search.pop(0)
            for _, lid, sub_i, guess, windows in self._covariance_candidates(q):
                n_cands += 1
                if windows is not None:
                    guess = self.b.search_global(self.submaps[sub_i], self.node_scans[q], self.bnb_mp, self.bnb_params, guess,
                                                 self.loop_scale, windows[0], windows[1])
                est, _cost = self.b.register_pair(self.submaps[sub_i], self.node_scans[q], self.loop_mp, guess)     # :395
                cs = self.b.cs_divergence(self.submaps[sub_i], self.node_scans[q], est)                             # :396-397
                added += self._close_loop(q, lid, sub_i, est, cs)
        self.loop_batches.append(n_cands)
        return added

    def _detect_loop_closures_covariance_batched(self):
        """The same search with the candidates of every pending query in one batch (they do not depend on each other: nodes and
        covariances only change in optimize_pose_graph): one batched global search, one batched refinement, one batched CS
        gate on the device, one read-back; log and edges in the sequential order."""
        cands = []
        while self.pending_loop_search:
            cands += self._covariance_candidates(self.pending_loop_search.pop(0))
        self.loop_batches.append(len(cands))
        if not cands:
            return 0
        search = None
        if self.compute_dfs:
            search = (self.bnb_mp, self.bnb_params, self.loop_scale, [c[4][0] for c in cands], [c[4][1] for c in cands])
        est, cs = self.b.loop_candidates_batch([self.submaps[c[2]] for c in cands], [self.node_scans[c[0]] for c in cands],
                                               np.array([c[3] for c in cands]), self.loop_mp, search)
        return sum(self._close_loop(c[0], c[1], c[2], est[p], cs[p]) for p, c in enumerate(cands))

    # ---- NDTSlam::optimizePoseGraph (ndt_slam.cpp:351-361) --------------------------------------
    def optimize_pose_graph(self):
        if not self.nodes or not self.edges or self.submap_idzs[-1] <= 0:
            return None
        n_nodes_per_submap = math.ceil((self.submap_size_poses - (self.smoothing_steps - 1)) / self.insertion_step)
        max_update_index = int((len(self.nodes) - 1) / n_nodes_per_submap) * n_nodes_per_submap
        x = np.array([[p[2], p[3], _angle(p)] for p in self.nodes])
        ia = np.array([e[0] for e in self.edges], dtype=np.int32)
        ib = np.array([e[1] for e in self.edges], dtype=np.int32)
        meas = np.array([[e[2][2], e[2][3], _angle(e[2])] for e in self.edges])
        sqi = np.array([e[3] for e in self.edges])
        xo, res = self.b.pose_graph_optimize(x, ia, ib, meas, sqi, max_update_index, self.pg_params)
        if self.loop_search == "covariance":
            # the ceres::Covariance block of global_fuser.cpp:62-87: at the optimised poses, the LAST pose constant (:68-69)
            try:
                cov = self.b.pose_graph_covariance(xo, ia, ib, meas, sqi, max_update_index, self.pg_params, -1)
            except Exception as e:                     # poses are still written back, covariances stay as they were
                self.n_covariance_failures += 1
                print("WARNING: pose graph covariance failed: %s" % e)
                cov = None
            if cov is not None:
                for i in range(len(self.nodes)):
                    c = cov[i]                         # cov_pos_pos, cov_pos_rot, cov_rot_rot -> Pose::cov (:86-89)
                    self.node_cov[i] = np.array([[c[0, 0], c[0, 1], c[0, 2]], [c[1, 0], c[1, 1], c[1, 2]], [c[0, 2], c[1, 2], c[2, 2]]])
        for i in range(len(self.nodes)):
            self.nodes[i] = _pose4(xo[i, 2], xo[i, 0], xo[i, 1])                          # Sophus::SE2d(rot, pos), global_fuser.cpp:85
        # LocalFuser::updateSubmaps (:65-88), pose part: the current submap's origin follows its root node
        self.current_global_transform = self.nodes[self.root_nodes[self.n_finished_submaps]].copy()
        self.n_optimizations += 1
        return res

    def node_positions(self):
        return np.array([[p[2], p[3], _angle(p)] for p in self.nodes])
