// Scans delivered as azimuth x range intensity rasters, through the C++ facade: RadarPreprocessor::filterPolarRaster /
// processPolarRaster and LocalFuser::processPolarRaster against the point-cloud overloads (filterScan / processScan /
// processPolarScan) on the EXPANSIONS of the same rasters -- x = ranges[b] * c_a, y = ranges[b] * s_a, z = 0, I = (float)v * scale,
// built here on the host as a converter would.  Everything must be equal: clouds, polar pairs, detections, cells, poses.
//
//   polar_raster_drive rasters.bin [--slam]
// rasters.bin: int32 n_scans, n_azimuths, n_bins; float intensity_scale; float cossin[n_azimuths][2]; float ranges[n_bins];
// uint8 raster[n_scans][n_azimuths][n_bins].  The rasters are handed over the way an Oxford radar PNG holds them: every row
// behind 11 bytes of metadata, so neither the start address nor the row pitch (n_bins + 11) is aligned to anything.
// --slam: the fusers keep keyframe clouds for the loop search (the path through filterPolarRaster instead of processPolarRaster).
// Prints one line per check and exits 0 when all hold.  tests/test_gpu_filter_raster_cpp.py runs it.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "randt_local_fuser.hpp"

using namespace randt;

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s rasters.bin [--slam]\n", argv[0]);
    return 2;
  }
  const bool slam = argc > 2 && std::string(argv[2]) == "--slam";
  std::ifstream in(argv[1], std::ios::binary);
  int32_t hdr[3] = {0, 0, 0};
  float scale = 1.f;
  in.read(reinterpret_cast<char*>(hdr), sizeof(hdr));
  in.read(reinterpret_cast<char*>(&scale), sizeof(scale));
  const int n_scans = hdr[0], n_az = hdr[1], n_bins = hdr[2];
  if (!in || n_scans <= 0 || n_az <= 0 || n_bins <= 0) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<float> cossin(static_cast<size_t>(n_az) * 2), ranges(static_cast<size_t>(n_bins));
  std::vector<unsigned char> dense(static_cast<size_t>(n_scans) * n_az * n_bins);
  in.read(reinterpret_cast<char*>(cossin.data()), static_cast<std::streamsize>(cossin.size() * sizeof(float)));
  in.read(reinterpret_cast<char*>(ranges.data()), static_cast<std::streamsize>(ranges.size() * sizeof(float)));
  in.read(reinterpret_cast<char*>(dense.data()), static_cast<std::streamsize>(dense.size()));
  if (!in) {
    std::fprintf(stderr, "%s is too short\n", argv[1]);
    return 2;
  }
  // the "PNG" rows and the expansions
  const size_t pitch = static_cast<size_t>(n_bins) + 11, image_bytes = pitch * n_az;
  std::vector<unsigned char> images(image_bytes * n_scans, 255);
  std::vector<float> clouds(static_cast<size_t>(n_scans) * n_az * n_bins * 4, 0.f);
  for (int s = 0; s < n_scans; ++s)
    for (int a = 0; a < n_az; ++a) {
      const unsigned char* row = &dense[(static_cast<size_t>(s) * n_az + a) * n_bins];
      std::memcpy(&images[s * image_bytes + a * pitch + 11], row, static_cast<size_t>(n_bins));
      for (int b = 0; b < n_bins; ++b) {
        float* p = &clouds[((static_cast<size_t>(s) * n_az + a) * n_bins + b) * 4];
        p[0] = ranges[b] * cossin[2 * a];
        p[1] = ranges[b] * cossin[2 * a + 1];
        p[3] = static_cast<float>(row[b]) * scale;
      }
    }
  randt_polar_raster desc{};
  desc.elem_type = RANDT_RASTER_U8;
  desc.n_azimuths = n_az;
  desc.n_bins = n_bins;
  desc.row_pitch_bytes = static_cast<int64_t>(pitch);
  desc.scan_pitch_bytes = static_cast<int64_t>(image_bytes);
  desc.intensity_scale = scale;

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

  // RadarPreprocessor, scan by scan
  RadarPreprocessor pre;
  RadarFilterParameters filt;
  filt.beam_distance_increment_threshold = 0.3f;
  pre.initialize(ctx, RadarPreprocessorParameters(), filt);
  NDTMapParameters mp;
  bool f_ok = true, p_ok = true;
  size_t kept = 0, cells = 0;
  for (int s = 0; s < n_scans; ++s) {
    const unsigned char* raster = &images[s * image_bytes + 11];
    const float* cloud = &clouds[static_cast<size_t>(s) * n_az * n_bins * 4];
    std::vector<float> out_r, out_c;
    std::vector<std::pair<double, double>> pol_r, pol_c;
    std::vector<std::array<double, 3>> det_r, det_c;
    f_ok = f_ok && pre.filterPolarRaster(raster, desc, cossin.data(), ranges.data(), out_r, pol_r, det_r) &&
           pre.filterScan(cloud, n_az, n_bins, 4, 3, out_c, pol_c, det_c);
    f_ok = f_ok && out_r.size() == out_c.size() && !out_r.empty() && std::memcmp(out_r.data(), out_c.data(), out_r.size() * sizeof(float)) == 0 &&
           pol_r == pol_c && det_r == det_c;
    kept += out_r.size() / 4;
    Map from_raster, from_cloud;
    from_raster.initialize(ctx, mp, 0.0, 0.0, 1024);
    from_cloud.initialize(ctx, mp, 0.0, 0.0, 1024);
    p_ok = p_ok && pre.processPolarRaster(raster, desc, cossin.data(), ranges.data(), from_raster) && pre.processScan(cloud, n_az, n_bins, 4, 3, from_cloud);
    const auto ca = from_raster.getCells(), cb = from_cloud.getCells();
    p_ok = p_ok && ca.size() == cb.size() && !ca.empty() && from_raster.getGridIndizes() == from_cloud.getGridIndizes();
    for (size_t i = 0; i < ca.size() && p_ok; ++i)
      p_ok = ca[i].getIntensityMean() == cb[i].getIntensityMean() && ca[i].getIntensityCov() == cb[i].getIntensityCov() && ca[i].getNumCells() == cb[i].getNumCells();
    cells += ca.size();
  }
  std::printf("%d scans of %d x %d: %zu kept points, %zu cells\n", n_scans, n_az, n_bins, kept, cells);
  report("filterPolarRaster vs filterScan", f_ok);
  report("processPolarRaster vs processScan", p_ok);

  // a duplicated azimuth: refused like the cloud it expands to, outputs untouched
  {
    std::vector<float> dup = cossin;
    dup[2 * 3] = dup[2 * 2];
    dup[2 * 3 + 1] = dup[2 * 2 + 1];
    std::vector<float> out(8, 1.f);
    std::vector<std::pair<double, double>> pol;
    std::vector<std::array<double, 3>> det;
    report("a duplicated azimuth is refused", n_az < 5 || (!pre.filterPolarRaster(&images[11], desc, dup.data(), ranges.data(), out, pol, det) && out.size() == 8));
  }

  // LocalFuser: the drive on rasters and on their expansions
  LocalFuserParameters lp;
  lp.filter_parameters = filt;
  if (slam) {
    lp.use_scan_context_as_loop_closure = true;
    lp.scan_context_parameters.PC_MAX_RADIUS = 20.0;
    lp.scan_context_parameters.SC_DIST_THRES = 0.5;
  }
  LocalFuser on_rasters, on_clouds;
  on_rasters.initialize(ctx, lp);
  on_clouds.initialize(ctx, lp);
  bool d_ok = true;
  SE2d last;
  for (int s = 0; s < n_scans; ++s) {
    on_rasters.processPolarRaster(&images[s * image_bytes + 11], desc, cossin.data(), ranges.data(), 0.25 * s);
    on_clouds.processPolarScan(&clouds[static_cast<size_t>(s) * n_az * n_bins * 4], n_az, n_bins, 4, 3, 0.25 * s);
    const SE2d a = on_rasters.getTransform(), b = on_clouds.getTransform();
    d_ok = d_ok && std::memcmp(a.d, b.d, sizeof(a.d)) == 0;
    last = a;
    std::printf("pose %d %.17g %.17g %.17g %.17g\n", s, a.d[0], a.d[1], a.d[2], a.d[3]);
  }
  report(slam ? "LocalFuser::processPolarRaster vs processPolarScan (slam)" : "LocalFuser::processPolarRaster vs processPolarScan", d_ok);
  report("the drive moved", last.d[2] != 0.0 || last.d[3] != 0.0);
  return all ? 0 : 1;
}
