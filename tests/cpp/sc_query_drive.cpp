// Place recognition for scans outside the database, through the C++ facade: SCManager::queryLoopClosure and
// SCManager::appendNode against the C entries (randt_sc_db_query, randt_sc_db_download / randt_sc_db_append_node,
// randt_sc_db_detect) on the same scans.  Ids, yaws and candidate lists must be equal.
//
//   sc_query_drive scans.bin
// scans.bin: int32 n_db, n_queries, n_points; float scans[n_db + n_queries][n_points][4] (x y z intensity);
// double pos[n_db + n_queries][2]; double dist[n_db + n_queries].  The first n_db scans become the database, the rest query it.
// Prints one line per check and exits 0 when all hold.  tests/test_gpu_sc_query_cpp.py runs it.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <vector>

#include "randt_facade.hpp"

using namespace randt;

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s scans.bin\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  int32_t hdr[3] = {0, 0, 0};
  in.read(reinterpret_cast<char*>(hdr), sizeof(hdr));
  const int n_db = hdr[0], n_q = hdr[1], n_pts = hdr[2], n_all = n_db + n_q;
  if (!in || n_db <= 0 || n_q <= 0 || n_pts <= 0) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<float> scans(static_cast<size_t>(n_all) * n_pts * 4);
  std::vector<double> pos(static_cast<size_t>(n_all) * 2), dist(static_cast<size_t>(n_all));
  in.read(reinterpret_cast<char*>(scans.data()), static_cast<std::streamsize>(scans.size() * sizeof(float)));
  in.read(reinterpret_cast<char*>(pos.data()), static_cast<std::streamsize>(pos.size() * sizeof(double)));
  in.read(reinterpret_cast<char*>(dist.data()), static_cast<std::streamsize>(dist.size() * sizeof(double)));
  if (!in) {
    std::fprintf(stderr, "%s is too short\n", argv[1]);
    return 2;
  }
  auto scan = [&](int i) { return &scans[static_cast<size_t>(i) * n_pts * 4]; };
  auto at = [&](int i) { return std::array<double, 2>{pos[2 * static_cast<size_t>(i)], pos[2 * static_cast<size_t>(i) + 1]}; };

  auto ctx = std::make_shared<Context>(0);
  if (last_status() != RANDT_OK) {
    std::printf("no HIP device: the drive cannot run (there is no CPU fallback)\n");
    return 3;
  }
  bool all = true;
  auto report = [&](const char* what, bool ok) {
    std::printf("%s: %s\n", what, ok ? "equal" : "DIFFERENT");
    all = all && ok;
  };

  ScanContextParameters sp;
  sp.PC_MAX_RADIUS = 20.0;
  sp.NUM_EXCLUDE_RECENT = 3;
  randt_sc_params p{};
  p.num_ring = sp.PC_NUM_RING;
  p.num_sector = sp.PC_NUM_SECTOR;
  p.max_radius = sp.PC_MAX_RADIUS;
  p.num_exclude_recent = sp.NUM_EXCLUDE_RECENT;
  p.num_candidates = sp.NUM_CANDIDATES_FROM_TREE;
  p.search_ratio = sp.SEARCH_RATIO;
  p.dist_thresh = sp.SC_DIST_THRES;
  p.assumed_drift = sp.assumed_drift;
  p.odom_eps = sp.odom_eps;
  p.odom_weight = sp.odom_weight;
  p.intensity_factor = sp.intensity_factor;
  const int k = p.num_candidates;

  // the same database twice: behind the facade, and behind the C handle
  SCManager mgr;
  mgr.initialize(ctx, sp);
  randt_sc_db* db = nullptr;
  if (randt_sc_db_create(ctx->get(), &p, 8, &db) != RANDT_OK) return 3;
  bool ok = true;
  for (int i = 0; i < n_db; ++i) {
    mgr.makeAndSaveScancontextAndKeys(scan(i), n_pts, 4, 3, at(i), dist[i]);
    ok = ok && randt_sc_db_append(db, scan(i), n_pts, 4, 3, &pos[2 * static_cast<size_t>(i)], dist[i], nullptr) == RANDT_OK;
  }
  report("both databases filled", ok && last_status() == RANDT_OK && mgr.size() == n_db && randt_sc_db_size(db) == n_db);

  // the database restored node by node from what the handle gives back
  SCManager restored;
  restored.initialize(ctx, sp);
  {
    std::vector<double> d(static_cast<size_t>(p.num_ring) * p.num_sector), rk(p.num_ring), sk(p.num_sector);
    for (int i = 0; i < n_db; ++i) {
      ok = ok && randt_sc_db_download(db, i, d.data(), rk.data(), sk.data()) == RANDT_OK;
      restored.appendNode(d.data(), rk.data(), sk.data(), at(i), dist[i]);
    }
  }
  report("appendNode restored every node", ok && last_status() == RANDT_OK && restored.size() == n_db);

  struct Answer {
    int id = -2;
    float yaw = -1.f;
    std::vector<int32_t> cid;
    std::vector<float> cyaw;
    std::vector<double> cdist;
  };
  auto c_query = [&](int i, bool prior) {
    Answer a;
    a.cid.assign(k, -7);
    a.cyaw.assign(k, -7.f);
    a.cdist.assign(k, -7.0);
    ok = ok && randt_sc_db_query(db, scan(i), n_pts, 4, 3, prior ? &pos[2 * static_cast<size_t>(i)] : nullptr, prior ? &dist[i] : nullptr, &a.id, &a.yaw,
                                 nullptr, a.cid.data(), a.cyaw.data(), a.cdist.data()) == RANDT_OK;
    return a;
  };
  auto same = [&](const Answer& a, const std::pair<int, float>& r, const SCManager::Candidates& c) {
    return a.id == r.first && std::memcmp(&a.yaw, &r.second, sizeof(float)) == 0 && a.cid == c.id &&
           std::memcmp(a.cyaw.data(), c.yaw.data(), sizeof(float) * k) == 0 && std::memcmp(a.cdist.data(), c.dist.data(), sizeof(double) * k) == 0;
  };
  bool q_ok = true, qp_ok = true, r_ok = true, bare_ok = true;
  int found = 0;
  for (int i = n_db; i < n_all; ++i) {
    SCManager::Candidates c;
    const Answer a = c_query(i, false);
    const auto r = mgr.queryLoopClosure(scan(i), n_pts, 4, 3, &c);
    q_ok = q_ok && same(a, r, c);
    bare_ok = bare_ok && mgr.queryLoopClosure(scan(i), n_pts, 4, 3) == r;
    const Answer ap = c_query(i, true);
    const auto rp = mgr.queryLoopClosure(scan(i), n_pts, 4, 3, at(i), dist[i], &c);
    qp_ok = qp_ok && same(ap, rp, c);
    SCManager::Candidates c2;
    const auto rr = restored.queryLoopClosure(scan(i), n_pts, 4, 3, at(i), dist[i], &c2);
    r_ok = r_ok && same(ap, rr, c2);
    found += a.id >= 0 ? 1 : 0;
    std::printf("query %d: id %d yaw %.9g | with prior: id %d yaw %.9g\n", i - n_db, a.id, a.yaw, ap.id, ap.yaw);
  }
  report("queryLoopClosure vs randt_sc_db_query", ok && q_ok);
  report("queryLoopClosure without the candidate list", bare_ok);
  report("queryLoopClosure with the odometry prior vs randt_sc_db_query", ok && qp_ok);
  report("the restored database answers queries like the original", ok && r_ok);
  report("some query found its place", found > 0);

  bool d_ok = true;
  for (int i = 0; i < n_db; ++i) {
    int id = -2;
    float yaw = -1.f;
    ok = ok && randt_sc_db_detect(db, i, &id, &yaw, nullptr) == RANDT_OK;
    const auto r = restored.detectLoopClosureID(i);
    d_ok = d_ok && r.first == id && std::memcmp(&r.second, &yaw, sizeof(float)) == 0;
  }
  report("the restored database answers detectLoopClosureID like the original", ok && d_ok);
  report("the queries left the databases as they were", mgr.size() == n_db && restored.size() == n_db && randt_sc_db_size(db) == n_db && last_status() == RANDT_OK);
  randt_sc_db_destroy(db);
  return all ? 0 : 1;
}
