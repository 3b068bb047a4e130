// A C++ caller of the pose-graph covariances through the facade (include/randt_facade.hpp, include/randt_local_fuser.hpp):
//
//   posegraph_cov_drive graph <graph.txt> <out.txt> <max_update_index> <compute_covariance 0|1>
//     GlobalFuser::optimizePoseGraph on a graph given as text -- "n e", n lines "x y rot", e lines
//     "id_begin id_end x y angle s0 .. s8" (sqrt-information row-major) -- with GlobalFuserParameters::compute_covariance
//     set or not.  out.txt: one line per node, "x y rot | cov_pos_pos[4] | cov_pos_rot[2] | cov_rot_rot | cov[9]", 17 digits.
//
//   posegraph_cov_drive drive <scans.bin> <poses.txt> <graph.txt> <submap_size_poses> <submap_overlap> <dfs 0|1> <mahalanobis>
//     LocalFuser with use_covariance_gated_loop_closure (the reference's loop search without Scan Context,
//     local_fuser.cpp:351-412) on a drive: loop search after every scan, GlobalFuser::optimizePoseGraph every 40 scans, like
//     tests/cpp/local_fuser_drive.cpp --slam.  scans.bin / poses.txt as there; graph.txt: "node x y rot", "loop query candidate cs
//     accepted", "edge id_begin id_end x y angle", "cov node c0 .. c8".
//
// tests/test_gpu_posegraph_cov_cpp.py runs both beside the C ABI and the Python harness (randt-slam_amd/slam.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "randt_local_fuser.hpp"

using namespace randt;

static int run_graph(int argc, char** argv) {
  if (argc < 6) return 2;
  std::ifstream in(argv[2]);
  int n = 0, e = 0;
  in >> n >> e;
  if (!in || n <= 0 || e < 0) return 2;
  std::map<int, Pose> nodes;
  for (int i = 0; i < n; ++i) {
    Pose p;
    in >> p.pos[0] >> p.pos[1] >> p.rot;
    p.pose = SE2d(p.rot, p.pos[0], p.pos[1]);
    nodes[i] = p;
  }
  std::vector<Constraint> edges(static_cast<size_t>(e));
  for (auto& c : edges) {
    double x, y, a;
    in >> c.id_begin >> c.id_end >> x >> y >> a;
    c.trans = SE2d(a, x, y);
    for (double& s : c.sqrt_information) in >> s;
  }
  if (!in) return 2;
  auto ctx = std::make_shared<Context>(0);
  if (last_status() != RANDT_OK) return 3;
  GlobalFuserParameters gp;
  gp.compute_covariance = std::atoi(argv[5]) != 0;
  GlobalFuser fuser;
  fuser.initialize(ctx, gp);
  std::mutex m;
  fuser.optimizePoseGraph(nodes, edges, m, std::atoi(argv[4]));
  std::FILE* out = std::fopen(argv[3], "w");
  if (!out) return 2;
  for (const auto& kv : nodes) {
    const Pose& p = kv.second;
    std::fprintf(out, "%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g", p.pos[0], p.pos[1], p.rot, p.cov_pos_pos[0], p.cov_pos_pos[1],
                 p.cov_pos_pos[2], p.cov_pos_pos[3], p.cov_pos_rot[0], p.cov_pos_rot[1], p.cov_rot_rot);
    for (double c : p.cov) std::fprintf(out, " %.17g", c);
    std::fprintf(out, "\n");
  }
  std::fclose(out);
  return first_error() == RANDT_OK ? 0 : 1;
}

static int run_drive(int argc, char** argv) {
  if (argc < 9) return 2;
  std::ifstream in(argv[2], std::ios::binary);
  int32_t n_scans = 0, n_points = 0;
  in.read(reinterpret_cast<char*>(&n_scans), 4);
  in.read(reinterpret_cast<char*>(&n_points), 4);
  if (!in || n_scans <= 0 || n_points <= 0) return 2;
  std::vector<float> scans(static_cast<size_t>(n_scans) * n_points * 4);
  in.read(reinterpret_cast<char*>(scans.data()), static_cast<std::streamsize>(scans.size() * sizeof(float)));
  if (!in) return 2;
  auto ctx = std::make_shared<Context>(0);
  if (last_status() != RANDT_OK) return 3;
  LocalFuserParameters lp;   // the indoor preset
  lp.submap_size_poses = std::atoi(argv[5]);
  lp.submap_overlap = std::atoi(argv[6]);
  lp.use_covariance_gated_loop_closure = true;
  lp.compute_dfs_loop_closure = std::atoi(argv[7]) != 0;
  lp.max_data_association_mahalanobis_dist = std::atof(argv[8]);
  lp.loop_closure_weight = 40.0;
  LocalFuser fuser;
  fuser.initialize(ctx, lp);
  std::FILE* out = std::fopen(argv[3], "w");
  if (!out) return 2;
  for (int i = 0; i < n_scans; ++i) {
    fuser.processScan(scans.data() + static_cast<size_t>(i) * n_points * 4, n_points, 4, 3, 0.25 * i);
    fuser.detectLoopClosures();
    if (i % 40 == 39) fuser.optimizePoseGraph();
    const SE2d p = fuser.getTransform();
    std::fprintf(out, "%.17g %.17g %.17g %.17g\n", p.d[0], p.d[1], p.d[2], p.d[3]);
  }
  std::fclose(out);
  std::FILE* g = std::fopen(argv[4], "w");
  if (!g) return 2;
  for (const auto& kv : fuser.nodes()) std::fprintf(g, "node %.17g %.17g %.17g\n", kv.second.pos[0], kv.second.pos[1], kv.second.rot);
  for (const auto& l : fuser.loopLog()) std::fprintf(g, "loop %d %d %.17g %d\n", l.query, l.candidate, l.cs, l.accepted ? 1 : 0);
  for (const auto& e : fuser.edges()) std::fprintf(g, "edge %d %d %.17g %.17g %.17g\n", e.id_begin, e.id_end, e.trans.d[2], e.trans.d[3], e.trans.angle());
  for (const auto& kv : fuser.nodes()) {
    std::fprintf(g, "cov %d", kv.first);
    for (double c : kv.second.cov) std::fprintf(g, " %.17g", c);
    std::fprintf(g, "\n");
  }
  std::fclose(g);
  std::printf("drive of %d scans done: %d submaps finished, first error status %d\n", n_scans, fuser.finishedSubmaps(), first_error());
  return first_error() == RANDT_OK ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "graph") == 0) return run_graph(argc, argv);
  if (argc >= 2 && std::strcmp(argv[1], "drive") == 0) return run_drive(argc, argv);
  std::fprintf(stderr, "usage: %s graph|drive ... (see the head of tests/cpp/posegraph_cov_drive.cpp)\n", argv[0]);
  return 2;
}
