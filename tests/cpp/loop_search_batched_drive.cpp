// A C++ caller of the covariance-gated loop search through the facade (include/randt_local_fuser.hpp), per candidate or batched:
//
//   loop_search_batched_drive <scans.bin> <graph.txt> <submap_size_poses> <submap_overlap> <mahalanobis> <detect_every>
//                             <optimise_every> <batched 0|1>
//     LocalFuser with use_covariance_gated_loop_closure and compute_dfs_loop_closure on a drive; every <detect_every> scans the
//     pending queries are searched with detectLoopClosuresCovarianceGated() (0) or detectLoopClosuresCovarianceGatedBatched() (1),
//     every <optimise_every> scans the pose graph is optimised.  scans.bin as tests/cpp/posegraph_cov_drive.cpp reads it;
//     graph.txt: "node x y rot", "loop query candidate cs accepted", "edge id_begin id_end x y angle", 17 digits.
//
// tests/test_gpu_loop_search_batched.py compares the two graph files byte for byte, and with the Python harness.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <vector>

#include "randt_local_fuser.hpp"

using namespace randt;

int main(int argc, char** argv) {
  if (argc < 9) {
    std::fprintf(stderr, "usage: see the head of tests/cpp/loop_search_batched_drive.cpp\n");
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
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
  lp.submap_size_poses = std::atoi(argv[3]);
  lp.submap_overlap = std::atoi(argv[4]);
  lp.use_covariance_gated_loop_closure = true;
  lp.compute_dfs_loop_closure = true;
  lp.max_data_association_mahalanobis_dist = std::atof(argv[5]);
  lp.loop_closure_weight = 40.0;
  const int detect_every = std::atoi(argv[6]), optimise_every = std::atoi(argv[7]);
  const bool batched = std::atoi(argv[8]) != 0;
  if (detect_every < 1 || optimise_every < 1) return 2;
  LocalFuser fuser;
  fuser.initialize(ctx, lp);
  double search_ms = 0.0;
  int largest_batch = 0;
  for (int i = 0; i < n_scans; ++i) {
    fuser.processScan(scans.data() + static_cast<size_t>(i) * n_points * 4, n_points, 4, 3, 0.25 * i);
    if (i % detect_every == detect_every - 1) {
      const auto t0 = std::chrono::steady_clock::now();
      if (batched) {
        int n = 0;
        fuser.detectLoopClosuresCovarianceGatedBatched(&n);
        if (n > largest_batch) largest_batch = n;
      } else {
        fuser.detectLoopClosuresCovarianceGated();
      }
      search_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (i % optimise_every == optimise_every - 1) fuser.optimizePoseGraph();
  }
  std::FILE* g = std::fopen(argv[2], "w");
  if (!g) return 2;
  for (const auto& kv : fuser.nodes()) std::fprintf(g, "node %.17g %.17g %.17g\n", kv.second.pos[0], kv.second.pos[1], kv.second.rot);
  for (const auto& l : fuser.loopLog()) std::fprintf(g, "loop %d %d %.17g %d\n", l.query, l.candidate, l.cs, l.accepted ? 1 : 0);
  for (const auto& e : fuser.edges()) std::fprintf(g, "edge %d %d %.17g %.17g %.17g\n", e.id_begin, e.id_end, e.trans.d[2], e.trans.d[3], e.trans.angle());
  std::fclose(g);
  std::printf("drive of %d scans (%s): %zu candidates, largest batch %d, loop search %.2f ms, first error status %d\n", n_scans,
              batched ? "batched" : "per candidate", fuser.loopLog().size(), largest_batch, search_ms, first_error());
  return first_error() == RANDT_OK ? 0 : 1;
}
