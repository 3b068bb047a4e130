// Exercises include/randt_facade.hpp the way LocalFuser::detectLoopClosures uses the reference
// classes (local_fuser.cpp:329-339): build two NDT maps from point clouds, then
// Matcher::estimateLoopConstraint.  Exit 0: pose recovered; 3: no GPU (expected on a CPU-only box).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <random>
#include <vector>

#include "randt_facade.hpp"

int main() {
  using namespace randt;
  // default error policy = the reference's: nothing throws, a failing call warns on std::cout and keeps the previous
  // value, the status is available from last_status()
  std::shared_ptr<Context> ctx = std::make_shared<Context>(0);
  if (!ctx->get()) {
    std::printf("no device: %s\n", randt_status_string(last_status()));
    // ... and with the throwing policy the same failure is an exception
    error_policy() = ErrorPolicy::kThrow;
    bool thrown = false;
    try {
      Context c2(0);
    } catch (const std::exception&) {
      thrown = true;
    }
    return thrown ? 3 : 5;
  }
  // scene: 40 tight blobs on a ring; "submap" scan at identity, "query" scan seen from (0.3, -0.2, 0.1 rad)
  std::mt19937 rng(7);
  std::normal_distribution<float> noise(0.f, 0.03f);
  std::uniform_real_distribution<float> uni(20.f, 80.f);
  const SE2d truth(0.1, 0.3, -0.2);
  const SE2d inv = truth.inverse();
  std::vector<float> fixed_pts, moving_pts;
  for (int b = 0; b < 40; ++b) {
    const float ang = 6.2831853f * b / 40.f, rad = 5.f + 3.f * ((b * 7) % 5) / 5.f;
    const float cx = rad * std::cos(ang) + 0.25f, cy = rad * std::sin(ang) + 0.25f, I0 = uni(rng);
    for (int k = 0; k < 20; ++k) {
      const float x = cx + noise(rng), y = cy + noise(rng), in = I0 + 10.f * noise(rng);
      fixed_pts.insert(fixed_pts.end(), {x, y, 0.f, in});
      const float mx = (float)(inv.d[0] * x - inv.d[1] * y + inv.d[2]);
      const float my = (float)(inv.d[1] * x + inv.d[0] * y + inv.d[3]);
      moving_pts.insert(moving_pts.end(), {mx + noise(rng) * 0.1f, my + noise(rng) * 0.1f, 0.f, in});
    }
  }
  NDTMapParameters mp;
  RadarPreprocessorParameters rp;
  Map scan_a, scan_b, submap;
  scan_a.initialize(ctx, mp, 0.0, 0.0, 512);
  scan_b.initialize(ctx, mp, 0.0, 0.0, 512);
  submap.initialize(ctx, mp, 0.0, 0.0);
  scan_a.addScan(fixed_pts.data(), (int)fixed_pts.size() / 4, 4, 3, rp);
  scan_b.addScan(moving_pts.data(), (int)moving_pts.size() / 4, 4, 3, rp);
  submap.mergeMapCell(scan_a);  // first scan of a submap (local_fuser.cpp:293)
  std::printf("submap cells %u, scan cells %u\n", submap.get_n_cells(), scan_b.get_n_cells());
  Map copy = submap;            // value semantics like the reference
  if (copy.get_n_cells() != submap.get_n_cells()) return 1;

  Matcher matcher;
  NDTMatcherParameters prm;
  matcher.initialize(prm);
  SE2d trans(0.05, 0.15, -0.05);  // initial guess
  randt_result st{};
  const double cost = matcher.estimateLoopConstraint(trans, submap, scan_b, 2, true, 1.5, &st);
  std::printf("pose %.5f %.5f %.5f  cost %.4f  residuals %d  iterations %d\n", trans.d[2], trans.d[3], trans.angle(), cost,
              st.n_residuals, st.iterations);
  const bool ok = std::fabs(trans.d[2] - 0.3) < 0.02 && std::fabs(trans.d[3] + 0.2) < 0.02 && std::fabs(trans.angle() - 0.1) < 0.01;
  // empty moving map: warning + pose untouched
  Map empty;
  empty.initialize(ctx, mp, 0.0, 0.0, 16);
  SE2d keep(0.2, 1.0, 2.0);
  matcher.estimateLoopConstraint(keep, submap, empty, 2, true, 1.5);
  const bool kept = keep.d[2] == 1.0 && keep.d[3] == 2.0;
  // fixed-lag odometry through the facade: predictTransform + estimateTransformCeres on a 3-scan drive, called with THE
  // REFERENCE'S SIGNATURE (std::deque<Map> fixed / moving windows, all parameters from initialize()) like
  // LocalFuser::processScan does (local_fuser.cpp:125-138), and -- same drive -- through the batch-slot variant
  bool win_ok = true;
  {
    Map sub_w;
    sub_w.initialize(ctx, mp, 0.0, 0.0);
    sub_w.mergeMapCell(scan_a);
    std::deque<Map> f_maps, map_window;
    f_maps.push_back(sub_w);
    std::vector<State> trajectory(1), trajectory_b(1);
    trajectory[0].lin_vel = {0.8, 0.0};
    trajectory_b[0].lin_vel = {0.8, 0.0};
    Matcher mw, mb;
    mw.initialize(prm);
    mb.initialize(prm);
    randt_map_params rmp{mp.size_x, mp.size_y, mp.resolution, 0.0, 0.0, mp.max_neighbour_manhattan_distance, mp.min_points_per_cell, 0};
    randt_maps *fixed_batch = nullptr, *scan_batch = nullptr;
    if (randt_maps_create(ctx->get(), 1, &rmp, 10000, 1, &fixed_batch) || randt_maps_create(ctx->get(), 4, &rmp, 512, 0, &scan_batch)) return 4;
    randt_cluster_params cp{rp.n_clusters, (float)rp.max_range};
    randt_ndt_build(ctx->get(), fixed_pts.data(), (int)fixed_pts.size() / 4, 4, 3, &cp, scan_batch, 0);
    const double id[4] = {1, 0, 0, 0};
    randt_maps_merge(fixed_batch, 0, scan_batch, 0, 1, id);
    SE2d cur, cur_b;
    std::vector<int32_t> window;
    for (int step = 1; step <= 4; ++step) {
      std::vector<float> pts;   // the blob scene seen from a sensor moving +0.25 m in x per step
      for (size_t p = 0; p < fixed_pts.size(); p += 4) pts.insert(pts.end(), {fixed_pts[p] - 0.25f * step, fixed_pts[p + 1], 0.f, fixed_pts[p + 3]});
      Map scan_w;
      scan_w.initialize(ctx, mp, 0.0, 0.0, 512);
      scan_w.addScan(pts.data(), (int)pts.size() / 4, 4, 3, rp);
      map_window.push_back(scan_w);
      const double stamp = 0.25 * step, yaw = 0.0;
      mw.predictTransform(yaw, stamp, trajectory);
      mw.estimateTransformCeres(cur, trajectory, yaw, stamp, f_maps, map_window);                 // reference signature
      if ((int)map_window.size() >= prm.smoothing_steps) map_window.pop_front();                   // local_fuser.cpp:152-154
      // batch-slot variant on the same data
      randt_ndt_build(ctx->get(), pts.data(), (int)pts.size() / 4, 4, 3, &cp, scan_batch, step % 4);
      window.push_back(step % 4);
      mb.predictTransform(yaw, stamp, trajectory_b);
      mb.estimateTransformCeres(cur_b, trajectory_b, yaw, stamp, fixed_batch, {0}, scan_batch, window, ctx->get(), mb.window_params());
      if ((int)window.size() >= prm.smoothing_steps) window.erase(window.begin());
      std::printf("step %d pose %.4f %.4f %.4f vel %.3f\n", step, cur.d[2], cur.d[3], cur.angle(), trajectory.back().lin_vel[0]);
      win_ok = win_ok && std::fabs(cur.d[2] - 0.25 * step) < 0.03 && std::fabs(cur.d[3]) < 0.03 && std::fabs(cur.angle()) < 0.01;
      win_ok = win_ok && cur.d[2] == cur_b.d[2] && cur.d[3] == cur_b.d[3] && cur.d[0] == cur_b.d[0];   // staging copies change nothing
    }
    randt_maps_destroy(fixed_batch);
    randt_maps_destroy(scan_batch);
  }
  // loop-closure gate and global search through the facade (local_fuser.cpp:338-339, :370-386).  The reference skips
  // cells with det(cov) < 1e-5 (ndt_map.cpp:47), so the gate gets broader blobs than the registration scene.
  bool gate_ok = true;
  {
    std::normal_distribution<float> wide(0.f, 0.15f), inoise(0.f, 2.f);
    std::vector<float> pa, pb;
    for (int b = 0; b < 40; ++b) {
      const float ang = 6.2831853f * b / 40.f, rad = 5.f + 3.f * ((b * 7) % 5) / 5.f;
      const float cx = rad * std::cos(ang) + 0.25f, cy = rad * std::sin(ang) + 0.25f, I0 = 20.f + (b * 13) % 60;
      for (int k = 0; k < 30; ++k) {
        pa.insert(pa.end(), {cx + wide(rng), cy + wide(rng), 0.f, I0 + inoise(rng)});
        pb.insert(pb.end(), {cx + wide(rng), cy + wide(rng), 0.f, I0 + inoise(rng)});
      }
    }
    Map fa, fb, sub2;
    fa.initialize(ctx, mp, 0.0, 0.0, 512);
    fb.initialize(ctx, mp, 0.0, 0.0, 512);
    sub2.initialize(ctx, mp, 0.0, 0.0);
    fa.addScan(pa.data(), (int)pa.size() / 4, 4, 3, rp);
    fb.addScan(pb.data(), (int)pb.size() / 4, 4, 3, rp);
    sub2.mergeMapCell(fa);
    const double cs_good = sub2.calculateCSDivergence(fb);   // same place
    Map off = fb;                                            // value copy, then transformMap like :338
    off.transformMap(SE2d(0.6, 1.5, -1.0));
    const double cs_bad = sub2.calculateCSDivergence(off);
    Matcher csm_matcher;
    NDTMatcherParameters csm_prm = prm;
    csm_prm.csm_cost_threshold = 1e9;       // csm_* come from the parameters, like in the reference (ndt_slam_parameters.h:76-83)
    csm_matcher.initialize(csm_prm);
    SE2d g(0.0, 0.0, 0.0);
    const double bnb_cost = csm_matcher.estimateTransformGlobalBNB(g, submap, scan_b, true, 1.5, 1.0, 0.3);   // reference signature
    std::printf("cs divergence aligned %.4f vs displaced %.4f; global search -> %.3f %.3f %.3f (cost %.4f)\n", cs_good, cs_bad, g.d[2],
                g.d[3], g.angle(), bnb_cost);
    // the correlative search is a coarse grid (0.1 m / finest level) over correspondences frozen at the guess
    gate_ok = cs_good < cs_bad && bnb_cost < 1e5 && std::fabs(g.d[2] - 0.3) < 0.5 && std::fabs(g.d[3] + 0.2) < 0.5 && std::fabs(g.angle() - 0.1) < 0.2;
  }
  // loop-closure candidates through the SCManager mirror: 20 keyframes on a line, the last one back at keyframe 2
  bool sc_ok = true;
  {
    ScanContextParameters scp;
    scp.PC_MAX_RADIUS = 12.0;
    scp.NUM_EXCLUDE_RECENT = 5;
    SCManager sc;
    sc.initialize(ctx, scp);
    for (int kf = 0; kf < 20; ++kf) {
      const double ox = kf == 19 ? 2 * 0.8 : kf * 0.8;  // sensor position along x
      std::vector<float> pts;
      for (size_t i = 0; i < fixed_pts.size(); i += 4)
        pts.insert(pts.end(), {fixed_pts[i] - (float)ox, fixed_pts[i + 1], 0.f, fixed_pts[i + 3]});
      sc.makeAndSaveScancontextAndKeys(pts.data(), (int)pts.size() / 4, 4, 3, {ox, 0.0}, kf * 0.8);
    }
    const auto early = sc.detectLoopClosureID(3);   // node_id < NUM_EXCLUDE_RECENT + 1
    const auto hit = sc.detectLoopClosureID(19);
    std::printf("scan context: %d nodes, query 19 -> %d (yaw %.3f)\n", sc.size(), hit.first, hit.second);
    sc_ok = sc.size() == 20 && early.first == -1 && hit.first == 2;
  }
  // cell-by-cell Map API: insertCluster / insertCell / coordinateToIndex / getClosestCells
  bool edit_ok = true;
  {
    Map m;
    m.initialize(ctx, mp, 0.0, 0.0, 64);
    std::vector<float> blob;
    for (int i = 0; i < 30; ++i) blob.insert(blob.end(), {3.1f + 0.01f * (i % 6), 1.2f + 0.012f * (i / 6), 0.f, 40.f + (i % 5)});
    m.insertCluster(blob.data(), 30, 4, 3);
    std::vector<float> blob2(blob);
    for (size_t i = 0; i < blob2.size(); i += 4) blob2[i] += 1.0f;
    m.insertCluster(blob2.data(), 30, 4, 3);
    m.insertCluster(blob.data(), 5, 4, 3);  // below the acceptance gate
    const auto cells = m.getCells();
    const auto grid = m.getGridIndizes();
    std::vector<size_t> near_pt, near_cell;
    m.getClosestCells(Vector2f{4.1f, 1.2f}, 2, near_pt);
    m.getClosestCells(cells.at(0), 1, near_cell);
    const int idx0 = (int)m.coordinateToIndex(cells.at(0).getMean());
    const int pos = m.insertCell(cells.at(0));
    std::printf("map edit: %u cells, slot of cell 0 -> %d, nearest to (4.1, 1.2): %zu, appended at %d\n", m.get_n_cells(), grid.at(idx0),
                near_pt.empty() ? (size_t)99 : near_pt[0], pos);
    edit_ok = cells.size() == 2 && grid.at(idx0) == 0 && near_pt.size() == 2 && near_pt[0] == 1 && near_cell.size() == 1 &&
              near_cell[0] == 0 && pos == 2 && m.get_n_cells() == 3;
    // a loop over the cells like NDTSlam::createVisualizationMsg's (ndt_slam.cpp:370-393): ONE download for the whole loop
    randt_pool_stats ps0{}, ps1{};
    randt_ctx_pool_stats(ctx->get(), &ps0);
    bool loop_ok = true;
    for (unsigned i = 0; i < 3; ++i) {
      Vector3f mu;
      Matrix3f cv;
      Vector2f mu2;
      Matrix2f cv2;
      loop_ok = loop_ok && m.getCellMeanAndCovariance(i, mu, cv) && m.getCellMeanAndCovariance(i, mu2, cv2) && m.getPointsInCell(i) == (i == 2 ? cells[0] : cells[i]).getNumCells() &&
                mu == (i == 2 ? cells[0] : cells[i]).getIntensityMean() && cv2 == (i == 2 ? cells[0] : cells[i]).getCov();
    }
    randt_ctx_pool_stats(ctx->get(), &ps1);
    std::printf("cell loop: ok %d, %lld stream waits for 9 accessor calls\n", loop_ok, static_cast<long long>(ps1.stream_syncs - ps0.stream_syncs));
    loop_ok = loop_ok && ps1.stream_syncs - ps0.stream_syncs <= 2;  // one download = the count, then the cells
    edit_ok = edit_ok && loop_ok;
    // Maps are VALUES (the reference copies them all over, local_fuser.cpp:128-136,173-178): copies share their storage until one
    // is written, and no write to one is ever seen through another
    Map copy = m, third = m;
    const bool shared = copy.handle() == m.handle() && third.handle() == m.handle();          // three values, one device batch
    copy.transformMap(SE2d(0.4, 2.0, -1.0));                                                    // the copy detaches and moves ...
    const auto moved = copy.getCells(), still = m.getCells();
    const bool detached = copy.handle() != m.handle() && third.handle() == m.handle() && moved.size() == 3 && still.size() == 3 &&
                          still[0].getMean() == cells[0].getMean() && moved[0].getMean() != cells[0].getMean();  // ... the original does not
    m.clear();                                                                                  // the original is written: `third` keeps the content
    const bool kept = m.get_n_cells() == 0 && m.isEmpty() && third.get_n_cells() == 3 && !third.isEmpty() && third.getCells()[1].getMean() == cells[1].getMean();
    Map fourth = third;
    fourth.insertCluster(blob2.data(), 30, 4, 3);                                               // a write to the newest copy
    const bool grew = fourth.get_n_cells() == 4 && third.get_n_cells() == 3 && copy.get_n_cells() == 3;
    std::printf("map values: shared %d detached %d kept %d grew %d\n", shared, detached, kept, grew);
    edit_ok = edit_ok && shared && detached && kept && grew;
  }
  // RadarPreprocessor: filterScan / processScan on a raw polar scan in host memory (a small one: 12 azimuths x 80 bins)
  bool pre_ok = true;
  {
    const int n_az = 12, n_bins = 80;
    std::vector<float> raw(static_cast<size_t>(n_az) * n_bins * 4, 0.f);
    for (int a = 0; a < n_az; ++a) {
      const double az = -M_PI + (a + 0.5) * (2 * M_PI / n_az);
      for (int b = 0; b < n_bins; ++b) {
        const double r = (b + 0.5) * 0.16;
        float* p = &raw[(static_cast<size_t>(a) * n_bins + b) * 4];
        p[0] = static_cast<float>(r * std::cos(az));
        p[1] = static_cast<float>(r * std::sin(az));
        p[3] = 1.0f + 0.01f * ((a * 7 + b * 3) % 5);
      }
      const int c = 20 + 3 * a;  // a peak of five bins per azimuth
      const float peak[5] = {30.f, 40.f, 50.f, 40.f, 30.f};
      for (int k = 0; k < 5; ++k) raw[(static_cast<size_t>(a) * n_bins + c - 2 + k) * 4 + 3] = peak[k];
    }
    RadarPreprocessor pre;
    RadarPreprocessorParameters clu;
    pre.initialize(ctx, clu, RadarFilterParameters());
    std::vector<float> cloud;
    std::vector<std::pair<double, double>> polar;
    std::vector<std::array<double, 3>> maxd;
    const bool f_ok = pre.filterScan(raw.data(), n_az, n_bins, 4, 3, cloud, polar, maxd);
    // the last azimuth is never flushed (radar_preprocessor.cpp:56-75): 11 detections, 5 kept points each
    bool peak_in = false;
    for (size_t i = 0; i < cloud.size() / 4 && i < 5; ++i) peak_in = peak_in || cloud[4 * i + 3] == 50.f;   // azimuth 0's run holds its peak
    pre_ok = f_ok && maxd.size() == 11 && cloud.size() / 4 >= 11 && polar.size() == cloud.size() / 4 && maxd[0][2] == 50.0 && peak_in;
    Map from_raw, from_pts;
    from_raw.initialize(ctx, mp, 0.0, 0.0, 64);
    from_pts.initialize(ctx, mp, 0.0, 0.0, 64);
    const bool p_ok = pre.processScan(raw.data(), n_az, n_bins, 4, 3, from_raw);
    RadarPreprocessorParameters rp;
    from_pts.addScan(cloud.data(), static_cast<int>(cloud.size() / 4), 4, 3, rp);
    const auto ca = from_raw.getCells(), cb = from_pts.getCells();
    pre_ok = pre_ok && p_ok && ca.size() == cb.size();
    for (size_t i = 0; i < ca.size() && pre_ok; ++i) pre_ok = ca[i].getIntensityMean() == cb[i].getIntensityMean() && ca[i].getIntensityCov() == cb[i].getIntensityCov();
    raw[(3 * n_bins + 40) * 4 + 0] = raw[(9 * n_bins + 40) * 4 + 0];  // a foreign point inside azimuth 3: refused, outputs untouched
    raw[(3 * n_bins + 40) * 4 + 1] = raw[(9 * n_bins + 40) * 4 + 1];
    const size_t before = cloud.size();
    pre_ok = pre_ok && !pre.filterScan(raw.data(), n_az, n_bins, 4, 3, cloud, polar, maxd) && cloud.size() == before;
    std::printf("radar preprocessor: %zu detections, %zu kept points, %zu cells from the raw scan\n", maxd.size(), cloud.size() / 4, ca.size());
  }
  // Cell mutators through the facade (ndt_cell.h:24-154) and the never-throw behaviour
  bool cell_ok = true;
  {
    std::vector<float> a, b;
    for (int i = 0; i < 24; ++i) a.insert(a.end(), {2.0f + 0.02f * (i % 6), 1.0f + 0.03f * (i / 6), 0.f, 30.f + (i % 7)});
    for (int i = 0; i < 12; ++i) b.insert(b.end(), {2.3f + 0.015f * (i % 4), 1.1f + 0.02f * (i / 4), 0.f, 50.f + (i % 3)});
    Cell c1, c2, c3;
    c1.initialize(ctx, mp.min_points_per_cell);
    c2.initialize(ctx, mp.min_points_per_cell);
    c3.initialize(ctx, mp.min_points_per_cell);
    const bool few = c1.addPointCloud(a.data(), 4, 4, 3);            // 4 points: below the gate, nothing happens
    const bool t1 = c1.addPointCloud(a.data(), 24, 4, 3);
    const bool t2 = c2.addPointCloud(b.data(), 12, 4, 3);
    for (int i = 0; i < 24; ++i) c3.addPoint(a[4 * i], a[4 * i + 1], a[4 * i + 3]);
    c3.updateCell();                                                  // addPoint ... updateCell == addPointCloud
    const bool same = c3.getNumCells() == 24 && c3.getMean() == c1.getMean() && c3.getIntensityCov() == c1.getIntensityCov();
    const double d3 = c1.mahalanobisSquaredIntensity(c2), d3r = c2.mahalanobisSquaredIntensity(c1), d2 = c1.mahalanobisSquared(c2);
    Cell sum = c1;
    sum += c2;                                                        // operator+=
    Cell rec = c1;
    rec.addPointCloud(b.data(), 12, 4, 3);                            // recursive update of a filled cell (+ regularisation)
    Cell moved = c1;
    moved.transformCell(SE2d(0.5, 1.0, -2.0));
    // the generating points travel with transformCellWithPointCloud (getPointCloud / getAngleDists, ndt_cell.h:146-154)
    Cell withpts = c1;
    withpts.transformCellWithPointCloud(SE2d(0.5, 1.0, -2.0));
    const auto& cloud0 = c1.getPointCloud();
    const auto& cloud1 = withpts.getPointCloud();
    bool cloud_ok = cloud0.size() == 24 * 4 && cloud1.size() == 24 * 4 && c1.getAngleDists().size() == 24 && withpts.getMean() == moved.getMean();
    for (int i = 0; i < 24 && cloud_ok; ++i) {
      const double px = std::cos(0.5) * cloud0[4 * i] - std::sin(0.5) * cloud0[4 * i + 1] + 1.0;
      const double py = std::sin(0.5) * cloud0[4 * i] + std::cos(0.5) * cloud0[4 * i + 1] - 2.0;
      cloud_ok = std::fabs(cloud1[4 * i] - px) < 1e-5 && std::fabs(cloud1[4 * i + 1] - py) < 1e-5 && cloud1[4 * i + 3] == cloud0[4 * i + 3];
    }
    const auto m0 = c1.getMean(), m1 = moved.getMean();
    const double ex = std::cos(0.5) * m0[0] - std::sin(0.5) * m0[1] + 1.0, ey = std::sin(0.5) * m0[0] + std::cos(0.5) * m0[1] - 2.0;
    std::printf("cells: n %zu + %zu -> %zu (recursive %zu), d3 %.4f (%.4f reversed) d2 %.4f, moved mean (%.4f, %.4f)\n", c1.getNumCells(),
                c2.getNumCells(), sum.getNumCells(), rec.getNumCells(), d3, d3r, d2, m1[0], m1[1]);
    cell_ok = !few && t1 && t2 && same && c1.getNumCells() == 24 && sum.getNumCells() == 36 && rec.getNumCells() == 36 && d3 > 0 &&
              std::fabs(d3 - d3r) < 1e-3 * d3 && d2 > 0 && std::fabs(m1[0] - ex) < 1e-4 && std::fabs(m1[1] - ey) < 1e-4 &&
              sum.getMean()[0] > m0[0] && sum.getMean()[0] < c2.getMean()[0] && moved.getNumCells() == 24 && cloud_ok;
    // never-throw: a registration with an impossible parameter set warns and leaves the pose as it was
    Matcher bad;
    NDTMatcherParameters bp = prm;
    bp.gnc_control_parameter_divisor = 0.5;                           // would hang the device loop: rejected by the ABI
    bad.initialize(bp);
    SE2d keep2(0.3, 4.0, 5.0);
    bad.estimateLoopConstraint(keep2, submap, scan_b, 2, true, 1.5);
    Map tiny;
    tiny.initialize(ctx, mp, 0.0, 0.0, 1);
    tiny.insertCluster(a.data(), 24, 4, 3);
    tiny.insertCluster(b.data(), 12, 4, 3);                           // capacity exhausted: map unchanged, no exception; the insert is
                                                                      // asynchronous, so the warning arrives with the next read of the map
    const bool tiny_one = tiny.get_n_cells() == 1 && last_status() == RANDT_ERR_UNSUPPORTED;   // the count is valid, the deferred status reported
    const bool tiny_again = tiny.get_n_cells() == 1 && last_status() == RANDT_OK;               // ... once
    cell_ok = cell_ok && keep2.d[2] == 4.0 && keep2.d[3] == 5.0 && tiny_one && tiny_again;
    // ... and when the first read behind a dropped cluster is the cell DOWNLOAD: the warning is printed, the
    // one cell that was placed is there -- not an empty vector cached for the map's current content
    Map tiny_dl;
    tiny_dl.initialize(ctx, mp, 0.0, 0.0, 1);
    tiny_dl.insertCluster(a.data(), 24, 4, 3);
    tiny_dl.insertCluster(b.data(), 12, 4, 3);
    const auto dl_cells = tiny_dl.getCells();
    const bool dl_reported = last_status() == RANDT_ERR_UNSUPPORTED;
    Vector3f dl_mean;
    Matrix3f dl_cov;
    const bool dl_ok = dl_cells.size() == 1 && dl_reported && dl_cells[0].getMean() == c1.getMean() && tiny_dl.getPointsInCell(0) == 24 &&
                       tiny_dl.getCellMeanAndCovariance(0, dl_mean, dl_cov) && dl_mean == c1.getIntensityMean() && tiny_dl.get_n_cells() == 1 &&
                       last_status() == RANDT_OK;
    if (!dl_ok) std::printf("download behind a deferred status: %zu cells, status reported %d\n", dl_cells.size(), (int)dl_reported);
    cell_ok = cell_ok && dl_ok;
    // HierarchicalMap pass-through: cluster by cluster == what insertCluster builds
    HierarchicalMap hm;
    hm.initialize(ctx, mp, 0.0, 0.0, 16);
    std::vector<float> both(a);
    both.insert(both.end(), b.begin(), b.end());
    hm.addClusters(both.data(), {0, 24, 36}, 4, 3);
    const auto hc = hm.getMap().getCells();
    cell_ok = cell_ok && hc.size() == 2 && hc[0].getMean() == c1.getMean() && hc[1].getIntensityCov() == c2.getIntensityCov();
    // HierarchicalMap::isEmpty() is the reference's FLAG (ndt_hierarchical_map.h:85-87): true from initialize() until the first
    // addClusters / mergeMapCell, whatever they held -- not the cell count; clear() leaves it alone; transformMapToOrigin / getOrigin
    // only keep the submap's origin (the cells do not move)
    HierarchicalMap fresh, target;
    fresh.initialize(ctx, mp, 0.0, 0.0, 16);
    target.initialize(ctx, mp, 0.0, 0.0, 16);
    const bool flag0 = fresh.isEmpty() && target.isEmpty() && fresh.getMap().isEmpty();
    target.mergeMapCell(fresh);                                       // merges NOTHING: no cell, yet the submap counts as started
    const bool flag1 = !target.isEmpty() && target.getMap().isEmpty() && target.getMap().get_n_cells() == 0;
    target.mergeMapCell(hm);
    const unsigned merged_cells = target.getMap().get_n_cells();      // (the two clusters may share a 0.5 m slot: then they merge into one cell)
    const bool flag2 = !target.isEmpty() && merged_cells >= 1 && merged_cells <= 2;
    target.clear();
    const bool flag3 = !target.isEmpty() && target.getMap().get_n_cells() == 0;
    target.transformMapToOrigin(SE2d(0.25, 3.0, -1.0));
    const bool origin_ok = target.getOrigin().d[2] == 3.0 && target.getOrigin().d[3] == -1.0 && std::fabs(target.getOrigin().angle() - 0.25) < 1e-15;
    if (!(flag0 && flag1 && flag2 && flag3 && origin_ok)) std::printf("HierarchicalMap flag / origin: %d %d %d %d %d\n", flag0, flag1, flag2, flag3, origin_ok);
    cell_ok = cell_ok && flag0 && flag1 && flag2 && flag3 && origin_ok;
  }
  // batched loop registration over a group of (virtual) GPUs: bit-identical to the pair-by-pair calls
  bool batch_ok = true;
  {
    const int n_cand = 7;
    std::vector<SE2d> guess, single;
    for (int p = 0; p < n_cand; ++p) guess.emplace_back(0.05 + 0.01 * p, 0.15 - 0.02 * p, -0.05 + 0.015 * p);
    single = guess;
    std::vector<double> single_cost;
    for (int p = 0; p < n_cand; ++p) single_cost.push_back(matcher.estimateLoopConstraint(single[p], p % 2 ? copy : submap, scan_b, 2, true, 1.5));
    for (int n_dev : {1, 3}) {
      DeviceGroup grp(std::vector<int>(n_dev, 0));              // n_dev contexts on device 0: peer-copy transport
      std::vector<SE2d> batch = guess;
      std::vector<const Map*> fixed_list{&submap, &copy}, moving_list(n_cand, &scan_b);
      std::vector<int> fixed_of(n_cand);
      for (int p = 0; p < n_cand; ++p) fixed_of[p] = p % 2;
      std::vector<randt_result> bst;
      const std::vector<double> bc = matcher.estimateLoopConstraintBatch(grp, batch, fixed_list, fixed_of, moving_list, 2, true, 1.5, &bst);
      for (int p = 0; p < n_cand; ++p)
        batch_ok = batch_ok && bc[p] == single_cost[p] && batch[p].d[0] == single[p].d[0] && batch[p].d[1] == single[p].d[1] &&
                   batch[p].d[2] == single[p].d[2] && batch[p].d[3] == single[p].d[3];
      std::printf("group of %d: %d candidates, pose[6] %.5f %.5f (single %.5f %.5f), transport %d\n", grp.size(), n_cand, batch[6].d[2],
                  batch[6].d[3], single[6].d[2], single[6].d[3], grp.transport());
    }
    // the group form checks fixed_of_pair like the one-context form: an index outside fixed_ndts is refused before anything is
    // staged or launched, every trans untouched; the same two small pairs with valid indices are the single calls' bit for bit
    {
      const int blob = 20 * 4, n_small = 5 * blob;   // five blobs = a few cells per map
      Map small_scan[2], small_fixed[2], small_moving[2];
      for (int i = 0; i < 2; ++i) {
        small_scan[i].initialize(ctx, mp, 0.0, 0.0, 64);
        small_scan[i].addScan(fixed_pts.data() + i * n_small, n_small / 4, 4, 3, rp);
        small_fixed[i].initialize(ctx, mp, 0.0, 0.0);
        small_fixed[i].mergeMapCell(small_scan[i]);
        small_moving[i].initialize(ctx, mp, 0.0, 0.0, 64);
        small_moving[i].addScan(moving_pts.data() + i * n_small, n_small / 4, 4, 3, rp);
      }
      const std::vector<SE2d> g2{SE2d(0.05, 0.15, -0.05), SE2d(0.08, 0.25, -0.15)};
      std::vector<SE2d> one = g2;
      double one_cost[2];
      for (int p = 0; p < 2; ++p) one_cost[p] = matcher.estimateLoopConstraint(one[p], small_fixed[p], small_moving[p], 2, true, 1.5);
      DeviceGroup grp(std::vector<int>(2, 0));
      const std::vector<const Map*> fixed_list{&small_fixed[0], &small_fixed[1]}, moving_list{&small_moving[0], &small_moving[1]};
      auto same_pose = [](const SE2d& a, const SE2d& b) { return std::memcmp(a.d, b.d, sizeof(a.d)) == 0; };
      bool refused[2];
      const std::vector<int> bad_index[2] = {{0, 2}, {-1, 0}};
      for (int t = 0; t < 2; ++t) {
        std::vector<SE2d> tr = g2;
        clear_errors();
        const std::vector<double> c = matcher.estimateLoopConstraintBatch(grp, tr, fixed_list, bad_index[t], moving_list, 2, true, 1.5);
        refused[t] = last_status() == RANDT_ERR_INVALID && c.size() == 2 && std::isnan(c[0]) && std::isnan(c[1]) && same_pose(tr[0], g2[0]) &&
                     same_pose(tr[1], g2[1]);
      }
      clear_errors();
      std::vector<SE2d> tr = g2;
      const std::vector<double> c = matcher.estimateLoopConstraintBatch(grp, tr, fixed_list, {0, 1}, moving_list, 2, true, 1.5);
      bool identical = last_status() == RANDT_OK && c.size() == 2;
      for (int p = 0; p < 2 && identical; ++p) identical = std::memcmp(&c[p], &one_cost[p], sizeof(double)) == 0 && same_pose(tr[p], one[p]);
      std::printf("group batch, fixed_of_pair out of range refused: %d %d, in range identical to the single calls: %d (%u + %u, %u + %u cells)\n",
                  (int)refused[0], (int)refused[1], (int)identical, small_fixed[0].get_n_cells(), small_moving[0].get_n_cells(),
                  small_fixed[1].get_n_cells(), small_moving[1].get_n_cells());
      batch_ok = batch_ok && refused[0] && refused[1] && identical;
    }
    // use_analytic_expressions_for_optimization: true -> the reference's hand-written functors on (pos, rot) blocks
    // (RANDT_PARAM_ANALYTIC: their inexact rotation Jacobian reproduced as written): converges next to the autodiff answer
    Matcher ana;
    NDTMatcherParameters ap = prm;
    ap.use_analytic_expressions_for_optimization = true;
    ana.initialize(ap);
    SE2d ta(0.05, 0.15, -0.05);
    clear_errors();
    randt_result sa{};
    const double c = ana.estimateLoopConstraint(ta, submap, scan_b, 2, true, 1.5, &sa);
    std::printf("analytic functors: pose %.5f %.5f %.5f cost %.4f iterations %d\n", ta.d[2], ta.d[3], ta.angle(), c, sa.iterations);
    batch_ok = batch_ok && std::isfinite(c) && first_error() == RANDT_OK && std::fabs(ta.d[2] - 0.3) < 0.02 && std::fabs(ta.d[3] + 0.2) < 0.02 &&
               std::fabs(ta.angle() - 0.1) < 0.01 && std::fabs(ta.d[0] * ta.d[0] + ta.d[1] * ta.d[1] - 1.0) < 1e-12;
    // a failing call: NaN, not a plausible cost; the first error stays readable
    Matcher bad2;
    NDTMatcherParameters bp2 = prm;
    bp2.gnc_control_parameter_divisor = 1.0;
    bad2.initialize(bp2);
    SE2d keep3(0.3, 4.0, 5.0);
    const double cb = bad2.estimateLoopConstraint(keep3, submap, scan_b, 2, true, 1.5);
    batch_ok = batch_ok && std::isnan(cb) && keep3.d[2] == 4.0 && last_status() == RANDT_ERR_INVALID && first_error() == RANDT_ERR_INVALID;
    clear_errors();
  }
  // pose-graph back end through the GlobalFuser mirror: a drifting square drive closed by one loop constraint
  bool pg_ok = true;
  {
    GlobalFuser gf;
    gf.initialize(ctx, GlobalFuserParameters{});
    std::map<int, Pose> nodes;
    std::vector<Constraint> edges;
    std::mutex mtx;
    const int n = 41;
    SE2d truth, drift;
    const double kPi = 3.14159265358979323846;
    for (int i = 0; i < n; ++i) {
      Pose p;
      p.pose = drift;
      p.pos = drift.translation();
      p.rot = drift.angle();
      nodes[i] = p;
      if (i + 1 == n) break;
      const SE2d step((i % 10 == 9) ? kPi / 2 : 0.0, 1.0, 0.0);      // 10 m sides, left turns: back at the start after 40 steps
      const SE2d noisy(step.angle() + 0.004, 1.0 + 0.01, 0.003);      // biased odometry
      Constraint c;
      c.id_begin = i;
      c.id_end = i + 1;
      c.trans = noisy;
      c.sqrt_information = {10, 0, 0, 0, 10, 0, 0, 0, 50};            // local_fuser.cpp:203-205
      edges.push_back(c);
      truth = truth * step;
      drift = drift * noisy;
    }
    Constraint loop;  // node 40 coincides with node 0
    loop.id_begin = 0;
    loop.id_end = n - 1;
    loop.trans = SE2d(0.0, 0.0, 0.0);
    loop.sqrt_information = {40, 0, 0, 0, 40, 0, 0, 0, 40};
    edges.push_back(loop);
    const auto before = nodes.at(n - 1).pos;
    gf.optimizePoseGraph(nodes, edges, mtx, n - 1);
    const auto after = nodes.at(n - 1).pos;
    const double e0 = std::hypot(before[0], before[1]), e1 = std::hypot(after[0], after[1]);
    std::printf("pose graph: end-point error %.3f m -> %.3f m, node 0 at (%.3f, %.3f)\n", e0, e1, nodes.at(0).pos[0], nodes.at(0).pos[1]);
    pg_ok = e1 < 0.1 * e0 && nodes.at(0).pos[0] == 0.0 && nodes.at(0).pos[1] == 0.0 &&
            std::fabs(nodes.at(n - 1).pose.d[2] - after[0]) < 1e-12;
  }
  std::printf("checks: pair %d kept %d window %d sc %d gate %d pg %d edit %d cell %d batch %d pre %d\n", ok, kept, win_ok, sc_ok, gate_ok, pg_ok, edit_ok, cell_ok, batch_ok, pre_ok);
  return (ok && kept && win_ok && sc_ok && gate_ok && pg_ok && edit_ok && cell_ok && batch_ok && pre_ok) ? 0 : 2;
}
