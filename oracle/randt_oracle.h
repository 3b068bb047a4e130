/*
 * randt_oracle.h -- CPU restatement ("oracle") of the RaNDT-SLAM NDT scan-matching hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the shipped library (randt-slam_amd/) links, imports or
 * calls this code; only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg do, and
 * only as the checker / reported CPU baseline.
 *
 * PARITY UNPINNED: the reference (IGMR-RWTH/RaNDT-SLAM) ships no tests, golden vectors or
 * fixtures for this path, and it cannot be compiled in this image (needs Eigen 3, Ceres 2.1.0,
 * Sophus 1.22.10, PCL, ROS noetic -- none present, no network).  This file therefore restates
 *   (1) the reference's first-party arithmetic, each function citing the file:line it follows
 *       (paths relative to /root/reference/ros/ndt_radar_slam/), and
 *   (2) the published algorithms of the un-vendored dependencies it calls on this path:
 *       Ceres Solver 2.1.0 (trust_region_minimizer.cc, levenberg_marquardt_strategy.cc,
 *       dense_qr_solver.cc, corrector.cc, loss_function.cc) and Sophus 1.22.10 (so2.hpp, se2.hpp,
 *       ceres_manifold.hpp), pinned in /root/reference/Dockerfile:11-27.
 * It is cross-checked by independent numerics in tests/ (finite differences, scipy least_squares,
 * zero-noise known-answer scenes, numpy float32 re-derivations) -- see tests/test_oracle_*.py.
 *
 * Where Eigen's exact fp32 operation order cannot be known without its sources (2x2 symmetric
 * eigen-solver, JacobiSVD inside Transform::rotation()), the oracle fixes a documented closed
 * form; those places are marked "SPEC DECISION".
 */
#ifndef RANDT_ORACLE_H
#define RANDT_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- cells / maps ------------- */

/* 48-byte NDT cell record: mean (x,y,intensity), upper triangle of the 3x3 covariance in the
 * field order of ndt_msgs/msg/Covariance.msg (xx,xy,xi,yy,yi,ii), point count.
 * Mirrors the numeric payload of rc::navigation::ndt::Cell (include/ndt_representation/ndt_cell.h:164-168). */
typedef struct orc_cell {
  float mean[3];
  float cov[6];
  uint32_t n;
  float max_intensity;
  uint32_t reserved;
} orc_cell;

/* Mirrors rc::navigation::ndt::Map (include/ndt_representation/ndt_map.h:155-166): compact cell
 * vector grid_ + dense index grid grid_indizes_ (-1 = empty). */
typedef struct orc_map {
  int32_t size_x, size_y;
  double res, offset_x, offset_y;
  double max_neighbour_dist;
  int32_t min_points;
  int32_t cap;
  int32_t n_cells;
  int32_t n_dropped; /* clusters whose slot was out of range (reference would throw, ndt_map.cpp:242) */
  orc_cell* cells;
  int32_t* grid;
} orc_map;

orc_map* orc_map_create(int size_x, int size_y, double res, double center_x, double center_y,
                        double max_neighbour_dist, int min_points, int cap);
void orc_map_destroy(orc_map* m);
void orc_map_clear(orc_map* m);
void orc_map_copy(orc_map* dst, const orc_map* src);

/* grid.cpp:7-14 */
void orc_grid_labels(const float* pts, int n, int stride, int ioff, int n_clusters, float max_range,
                     int32_t* labels);
/* radar_preprocessor.cpp:151-169 + ndt_hierarchical_map.cpp:28-33 + ndt_map.cpp:238-245 + ndt_cell.cpp:25-114 */
int orc_ndt_build(orc_map* m, const float* pts, int n, int stride, int ioff, int n_clusters,
                  float max_range);
int orc_ndt_build_pndt(orc_map* m, const float* pts, int n, int stride, int ioff, int n_clusters, float max_range,
                       const float* polar, const float* beam);
/* ndt_cell.cpp:36-114 (first-fill branch + regularisation) for one cluster of k points */
int orc_cell_from_points(orc_cell* c, const float* pts, const int32_t* idx, int k, int stride,
                         int ioff, int min_points);
int orc_cell_from_points_pndt(orc_cell* c, const float* pts, const int32_t* idx, int k, int stride, int ioff, int min_points,
                              const float* polar /* (angle, range) per point or NULL */, const float* beam /* 3x3 row-major */);
/* ndt_cell.h:133-142 */
void orc_cell_merge(orc_cell* dst, const orc_cell* src);
/* Cell::addPointCloud + updateCell incl. the recursive update of an already filled cell (ndt_cell.cpp:25-114) */
int orc_cell_update(orc_cell* c, const float* pts, int k, int stride, int ioff, int min_points);
/* Cell::mahalanobisSquared / mahalanobisSquaredIntensity (ndt_cell.cpp:158-169) */
double orc_cell_mahalanobis(const orc_cell* self, const orc_cell* subtrahend, int use_intensity);
/* Sophus SE2d::cast<float>() -> Eigen::Affine2f, as used at ndt_matcher.cpp:208, local_fuser.cpp:175 */
void orc_pose_to_affine_f(const double pose4[4], float aff[4]);
/* ndt_cell.cpp:117-123 */
void orc_cell_transform(orc_cell* c, const float aff[4]);
/* ndt_map.cpp:177-182 (leaves the index grid stale, like the reference) */
void orc_map_transform(orc_map* m, const float aff[4]);
/* ndt_map.cpp:191-207 */
void orc_map_merge(orc_map* fixed, const orc_map* moving);
/* ndt_map.h:87-90 */
uint32_t orc_map_coord_to_index(const orc_map* m, float x, float y);

/* ndt_matcher.cpp:200-215 + ndt_map.cpp:101-175 + ndt_cell.cpp:172-176.  corr is M x k, -1 padded.
 * returns total number of correspondences. */
int orc_associate(const orc_map* fixed, const orc_map* moving, const double pose4[4], int k,
                  int lookup_mahalanobis, int use_intensity, int32_t* corr);

/* ---------------------------------------------------------------- loss --------------------- */
/* ceres_loss_functions.cpp:19-39 (BarronLoss) wrapped in ceres::ScaledLoss(weight) */
void orc_barron_scaled(double s, double scale_a, double alpha, double mu, double weight,
                       double rho[3]);

/* ---------------------------------------------------------------- registration ------------- */

enum { ORC_PARAM_MANIFOLD = 0, ORC_PARAM_AMBIENT4 = 1, ORC_PARAM_VECTOR = 2, ORC_PARAM_ANALYTIC = 3 /* VECTOR blocks + the reference's analytic NDT functors */ };
enum { ORC_LINSOLVE_QR = 0, ORC_LINSOLVE_NORMAL = 1 };
enum {
  ORC_TERM_CONVERGENCE_FUNCTION = 1,
  ORC_TERM_CONVERGENCE_PARAMETER = 2,
  ORC_TERM_CONVERGENCE_GRADIENT = 3,
  ORC_TERM_CONVERGENCE_RADIUS = 4,
  ORC_TERM_NO_CONVERGENCE = 5,
  ORC_TERM_FAILURE = 6
};

typedef struct orc_matcher_params {
  double loss_scale;   /* 'a' of BarronLoss: loss_function_scale (odometry) or the `scale` arg (loop) */
  double mu_scale;     /* parameters_.loss_function_scale used in the gnc_mu formula (ndt_matcher.cpp:388,475) */
  double loss_alpha;   /* loss_function_convexity */
  double loss_weight;  /* ScaledLoss factor: ndt_weight/(n_cells*k) (ndt_matcher.cpp:392) or 1 (:479) */
  double gnc_divisor;
  int32_t gnc_steps;
  int32_t max_iterations;
  int32_t n_neighbours;
  int32_t lookup_mahalanobis;
  int32_t use_intensity;
  int32_t parameterization;
  int32_t linear_solver;
  int32_t max_consecutive_invalid_steps;
  /* Ceres 2.1.0 Solver::Options defaults (not overridden at ndt_matcher.cpp:372-379) */
  double function_tolerance, gradient_tolerance, parameter_tolerance;
  double initial_radius, max_radius, min_radius;
  double min_relative_decrease, min_lm_diagonal, max_lm_diagonal;
} orc_matcher_params;

void orc_matcher_params_default(orc_matcher_params* p);

#define ORC_TRACE_MAX 4096
typedef struct orc_solve_stats {
  int32_t n_residuals;
  int32_t n_solves;          /* GNC solves performed */
  int32_t n_iterations;      /* total minimizer iterations (incl. iteration 0 of each solve) */
  int32_t n_jac_evals;       /* residual+Jacobian evaluations */
  int32_t n_cost_evals;      /* residual-only evaluations */
  int32_t termination;       /* of the last solve */
  double initial_cost;       /* of the first solve */
  double final_cost;         /* summary.final_cost of the last solve */
  double max_raw_residual;
  double mu0;
  /* per-iteration trace across all solves */
  int32_t trace_len;
  double trace_cost[ORC_TRACE_MAX];
  double trace_radius[ORC_TRACE_MAX];
  int32_t trace_flag[ORC_TRACE_MAX]; /* 0 = iteration zero, 1 = accepted, 2 = rejected, 3 = invalid */
} orc_solve_stats;

/* One residual + Jacobian (ceres_residuals.h:454-552 through Ceres autodiff x Sophus manifold).
 * d = 2 or 3.  mm/fm: means (d), mc/fc: full dxd row-major covariances.  pose4 = [c,s,tx,ty].
 * jac (may be NULL): 3 entries for MANIFOLD / VECTOR, 4 for AMBIENT4.  Returns raw residual r. */
/* evaluations (with Jacobian) at which the sqrt(0) guard fired since the last reset (reset != 0 clears the count) */
long long orc_sqrt_zero_count(int reset);
double orc_ndt_residual(int d, int parameterization, const double* pose4, const double* mm,
                        const double* mc, const double* fm, const double* fc, double* jac);

/* GNC + LM for fixed correspondences (ndt_matcher.cpp:466-483 + Ceres LM).  corr M x k. */
int orc_solve_pair(const orc_map* fixed, const orc_map* moving, const int32_t* corr, int k,
                   const orc_matcher_params* p, double pose4[4], orc_solve_stats* st);

/* Matcher::estimateLoopConstraint (ndt_matcher.cpp:426-493): associate + solve.
 * Returns final_cost / num_residual_blocks through *cost_out. */
int orc_register_pair(const orc_map* fixed, const orc_map* moving, const orc_matcher_params* p,
                      double pose4[4], double* cost_out, orc_solve_stats* st);

/* Batch helper for the CPU baseline: B independent registrations (OpenMP over registrations
 * when compiled with -fopenmp).  points: B scans of n points; fixed_idx[b] selects the submap. */
int orc_register_batch(int B, const float* pts, int n, int stride, int ioff, int n_clusters,
                       float max_range, orc_map* const* fixed_maps, const int32_t* fixed_idx,
                       const orc_matcher_params* p, const double* guess4, double* pose4_out,
                       double* cost_out, int32_t* iters_out, int n_threads,
                       int32_t* stats_out /* nullable, [B][4]: n_residuals, n_solves, termination, passes */);

/* ---------------------------------------------------------------- fixed-lag window (a16/a17) */

/* rc::navigation::ndt::State (include/ndt_slam/trajectory_representation.h:12-22) as a POD. */
typedef struct orc_state {
  double pose[4]; /* Sophus::SE2d data: cos, sin, tx, ty */
  double pos[2];
  double rot;
  double lin_vel[2];
  double rot_vel;
  double lin_acc[2];
  double imu_bias;
  double stamp;
} orc_state;

typedef struct orc_window_params {
  double motion_sqrtI[64];  /* covariance_scaling_factor * motion_sqrtI, row-major 8x8 (ndt_matcher.cpp:99) */
  double ndt_weight, weight_imu, weight_imu_bias;
  double pose_reject_translation, pose_reject_rotation;
  int32_t smoothing_steps, use_imu, use_constant_velocity_model, reserved;
} orc_window_params;

/* Matcher::predictTransform, manifold branch (ndt_matcher.cpp:22-59) -> predictSE2 (ceres_residuals.h:62-83) */
void orc_predict_state(const orc_state* last, double stamp, orc_state* next);
/* ... and the (pos[2], rot) branch (optimize_on_manifold: false), ndt_matcher.cpp:27-41 with predict(), ceres_residuals.h:25-55 */
void orc_predict_state_vec(const orc_state* last, double stamp, orc_state* next);
/* MotionModelFactor / RotationalResidual on (pos, rot) blocks (ceres_residuals.h:554-619, 307-336); layouts as the SE2 forms */
void orc_motion_residual_vec(const orc_state* x0, const orc_state* x1, const double* sqrtI, double* r8, double* J8x16);
void orc_imu_residual_vec(const orc_state* x0, const orc_state* x1, double imu_rot, double weight, double bias_weight, double* r2,
                          double* J2x8);
/* MotionModelFactorSE2 (ceres_residuals.h:621-679): 8 residuals (already multiplied by sqrtI) and
 * the 8 x 16 row-major Jacobian w.r.t. tangent [X0: pose3 v2 w1 a2 | X1: pose3 v2 w1 a2]. */
void orc_motion_residual(const orc_state* x0, const orc_state* x1, const double* sqrtI, double* r8, double* J8x16);
/* RotationalResidualSE2 (ceres_residuals.h:338-370): 2 residuals, 2 x 8 Jacobian w.r.t.
 * [X0 pose3, X1 pose3, b0, b1]. */
void orc_imu_residual(const orc_state* x0, const orc_state* x1, double imu_rot, double weight, double bias_weight,
                      double* r2, double* J2x8);
/* Matcher::estimateTransformCeres (ndt_matcher.cpp:322-424).  states: n_states = S+1 (oldest first,
 * its pose constant); moving: S maps for states 1..S; fixed: n_fixed maps; imu: S constraints (pair j
 * = states j, j+1) or NULL.  trans4: in = prior pose for the rejection gate, out = newest pose.
 * returns 1 if the estimate was rejected (ndt_matcher.cpp:411-422), 0 otherwise, <0 on failure. */
int orc_register_window(orc_map* const* fixed, int n_fixed, orc_map* const* moving, orc_state* states, int n_states,
                        const double* imu, const orc_matcher_params* p, const orc_window_params* wp, double trans4[4],
                        orc_solve_stats* st);

/* ---------------------------------------------------------------- f-3: correlative search -- */
typedef struct orc_bnb_params {
  double csm_window_linear, csm_window_angular, csm_linear_step, csm_cost_threshold, csm_max_px_accurate_range;
  int32_t csm_n_iter, reserved;
} orc_bnb_params;
/* problem.Evaluate(apply_loss_function = true) at n_poses poses for one frozen correspondence set
 * (ndt_matcher.cpp:561-576): cost[p] = sum 1/2 rho(s) with BarronLoss(scale, alpha) (mu = 1, weight 1). */
void orc_eval_cost_batch(const orc_map* fixed, const orc_map* moving, const int32_t* corr, int k, int use_intensity,
                         double scale, double alpha, const double* poses4, int n_poses, double* cost, int* n_res);
/* Matcher::estimateTransformGlobalBNB (ndt_matcher.cpp:495-608).  trans4 in/out; returns min_cost.
 * n_evals (nullable): number of poses evaluated. */
double orc_search_global_bnb(const orc_map* fixed, const orc_map* moving, const orc_matcher_params* p, const orc_bnb_params* bp,
                             double scale, double search_window_linear, double search_window_angular, double trans4[4],
                             int* n_evals);

/* ---------------------------------------------------------------- f-2: CS divergence ------- */
/* Map::calculateCSDivergence (src/ndt_representation/ndt_map.cpp:42-99) of fixed vs moving (the
 * moving map already transformed, local_fuser.cpp:338-339).  SPEC DECISION: the reference's three
 * accumulators are uninitialised (:43-46); they start at 0 here.  terms (nullable): interaction,
 * fixed, moving. */
double orc_cs_divergence(const orc_map* fixed, const orc_map* moving, double terms[3]);

/* ---------------------------------------------------------------- f-1: filterScan ---------- */
typedef struct orc_filter_params {
  float min_range, max_range, min_intensity, beam_distance_increment_threshold;
  float sensor_to_base[12]; /* row-major 3x4 of initial_transform_radar_baselink_ */
} orc_filter_params;
/* RadarPreprocessor::filterScan (src/radar_preprocessing/radar_preprocessor.cpp:45-125), sequential,
 * exactly as written (incl. the never-flushed last azimuth and the carried-over max index).
 * raw: n points (stride floats, intensity at ioff), azimuth after azimuth, range ascending.
 * out_pts: capacity x 4 floats (x y z I, base frame), out_polar: capacity x 2 (angle, dist),
 * peaks: peak_cap x 3 (angle, dist, intensity) = max_detections.  Returns #filtered points (or -1 on
 * overflow); *n_peaks receives the number of max detections. */
int orc_filter_scan(const float* raw, int n, int stride, int ioff, const orc_filter_params* p, float* out_pts,
                    float* out_polar, int capacity, float* peaks, int peak_cap, int* n_peaks);

/* ---------------------------------------------------------------- f-4: Scan Context ------- */
/* SCManager (src/local_fuser/Scancontext/Scancontext.cpp:64-341, parameters ndt_slam.cpp:515-552): the
 * loop-closure candidate generator in front of estimateLoopConstraint (local_fuser.cpp:323).
 * SPEC DECISIONS: xy2theta calls the unqualified atan on a float -> the correctly rounded float arctangent; Eigen's .mean() /
 * .norm() / .dot() reduction order depends on the reference's build flags -> plain left-to-right sums here
 * (GPU parity is by tolerance); the nanoflann KD-tree search is restated as an exact brute-force kNN in float
 * (ties: lower index first); the tree is rebuilt on every query (TREE_MAKING_PERIOD = 1 semantics); an entry whose float
 * key distance to the query is not >= 0 (a NaN distance; +inf is a distance like any other) is never a candidate, and when no candidate is left the
 * remaining ranks are absent. */
typedef struct orc_sc_params {
  int num_ring, num_sector;          /* PC_NUM_RING, PC_NUM_SECTOR */
  double max_radius;                 /* PC_MAX_RADIUS */
  int num_exclude_recent, num_candidates;
  double search_ratio, dist_thresh, assumed_drift, odom_eps, odom_weight, intensity_factor;
} orc_sc_params;
/* makeScancontext (:156-204) + makeRingkey / makeSectorkey (:207-237).  pts: n points, stride floats, intensity at
 * ioff.  desc: [num_sector][num_ring] (Eigen column-major: one sector = one contiguous column); ring_key [num_ring],
 * sector_key [num_sector]. */
void orc_sc_make(const float* pts, int n, int stride, int ioff, const orc_sc_params* p, double* desc, double* ring_key,
                 double* sector_key);
/* distanceBtnScanContext (:115-152): returns the combined distance, *shift = argmin column shift. */
double orc_sc_distance(const orc_sc_params* p, const double* sc1, const double* sc2, const double pos1[2], const double pos2[2],
                       double dist1, double dist2, int* shift);
/* detectLoopClosureID (:261-341) for query node_id over a database of n_db nodes (desc [n_db][S*R], ring keys [n_db][R],
 * positions [n_db][2], traversed distances [n_db]).  Returns the loop id or -1; *yaw = relative yaw [rad] (float arithmetic
 * as in the reference), *min_dist (nullable) = best combined distance. */
int orc_sc_detect(const orc_sc_params* p, const double* desc, const double* ring_keys, const double* pos, const double* dist,
                  int n_db, int node_id, float* yaw, double* min_dist);

/* ---------------------------------------------------------------- f-4: pose graph ----------- */
/* GlobalFuser::optimizePoseGraph (src/global_fuser/global_fuser.cpp:13-105) with PoseGraph2dErrorTerm
 * (include/global_fuser/pose_graph_2d_error_term.h:33-80) and NormalizeAngle (include/ndt_registration/
 * state_manifold.h:17-23).  Ceres 2.1.0 trust-region LM, SPARSE_NORMAL_CHOLESKY restated as a dense Cholesky of the
 * same damped normal equations (same step up to rounding); optional HuberLoss with the Ceres corrector. */
typedef struct orc_pg_params {
  int32_t use_robust_loss;  /* GlobalFuserParameters::use_robust_loss -> ceres::HuberLoss(loss_function_scale) (:17-23) */
  int32_t max_iterations;   /* 200000 (:52) */
  int32_t max_consecutive_invalid_steps;
  int32_t reserved;
  double loss_scale;
  double function_tolerance, gradient_tolerance, parameter_tolerance;
  double initial_radius, max_radius, min_radius;
  double min_relative_decrease, min_lm_diagonal, max_lm_diagonal;
} orc_pg_params;
typedef struct orc_pg_result {
  double initial_cost, final_cost;
  int32_t iterations, termination, n_residual_blocks, n_loop_closures;
} orc_pg_result;
void orc_pg_params_default(orc_pg_params* p);
/* residual (3) and the 3x3 Jacobians w.r.t. (x_a, y_a, yaw_a) and (x_b, y_b, yaw_b), sqrt-information applied, no loss */
void orc_pg_edge(const double pose_a[3], const double pose_b[3], const double meas[3], const double sqrt_info[9], double r[3],
                 double Ja[9], double Jb[9]);
/* poses [n_poses][3] = (pos.x, pos.y, rot), in/out; edges: id_begin/id_end, meas [E][3] = (trans.translation(), trans.log()(2)),
 * sqrt_info [E][9] row-major.  Edge e is used iff id_begin+1 == id_end || id_end <= max_update_index (:32); pose 0 is
 * constant (:48-49).  Returns 0 on success. */
int orc_pose_graph_optimize(int n_poses, double* poses, int n_edges, const int32_t* id_begin, const int32_t* id_end,
                            const double* meas, const double* sqrt_info, int max_update_index, const orc_pg_params* p,
                            orc_pg_result* out);

/* ---------------------------------------------------------------- SE(2) helpers (Sophus) --- */
void orc_se2_exp(const double xi[3], double out4[4]);
void orc_se2_log(const double p4[4], double xi[3]);
void orc_se2_mul(const double a4[4], const double b4[4], double out4[4]);
void orc_se2_inv(const double a4[4], double out4[4]);

int orc_num_threads(void);
/* timing only: OpenMP threads over the residual blocks of ONE problem (Ceres' options.num_threads); default 1 = sequential sums */
void orc_set_eval_threads(int n);

#ifdef __cplusplus
}
#endif
#endif
