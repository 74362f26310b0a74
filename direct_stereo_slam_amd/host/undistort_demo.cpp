// undistort_demo -- the node's image hand-over through the C++ adaptor (Undistort.hpp): raw mono8 camera bytes of one camera
// file in, the tracker's level-0 plane out.
//   undistort_demo camera.txt raw.u8 out.f32 [w_out h_out [G.f32 [vignette_inv.f32]]]
// raw.u8: W x H bytes of the camera file's second line; out.f32: the w_out x h_out intensities of level 0; G.f32: 256 floats,
// vignette_inv.f32: W x H floats.  Prints one JSON line (output size and camera).
#include <cstdio>
#include <vector>

#include "TrackerAndScaler.hpp"
#include "Undistort.hpp"

static bool read_file(const char *path, void *dst, size_t bytes) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  const bool ok = fread(dst, 1, bytes, f) == bytes;
  fclose(f);
  return ok;
}

int main(int argc, char **argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s camera.txt raw.u8 out.f32 [w_out h_out [G.f32 [vignette_inv.f32]]]\n", argv[0]);
    return 2;
  }
  dsm_context *ctx = nullptr;
  if (dsm_context_create(0, &ctx) != DSM_OK) {
    fprintf(stderr, "dsm_context_create: %s\n", dsm_last_error());
    return 3;
  }
  try {
    const dsm_host::CameraFile cf = dsm_host::readCameraFile(argv[1]);
    const int w_out = argc > 5 ? atoi(argv[4]) : 0, h_out = argc > 5 ? atoi(argv[5]) : 0;
    std::vector<float> G(256), vig((size_t)cf.w_in * cf.h_in);
    const bool haveG = argc > 6, haveVig = argc > 7;
    if (haveG && !read_file(argv[6], G.data(), G.size() * sizeof(float))) throw std::runtime_error("cannot read G");
    if (haveVig && !read_file(argv[7], vig.data(), vig.size() * sizeof(float))) throw std::runtime_error("cannot read vignette");
    std::vector<uint8_t> raw((size_t)cf.w_in * cf.h_in);
    if (!read_file(argv[2], raw.data(), raw.size())) throw std::runtime_error("cannot read the raw image");
    {
      dsm_host::Undistort und(ctx, argv[1], haveG ? G.data() : nullptr, haveVig ? vig.data() : nullptr, w_out, h_out);
      int w, h;
      und.getSize(w, h);
      const std::vector<double> T = {1, 0, 0, -0.5372, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      dsm_host::TrackerAndScaler trk(ctx, w, h, 1, T, und.getK());
      trk.makeK(und.getK()[0], und.getK()[1], und.getK()[2], und.getK()[3]);
      und.uploadImage(trk, DSM_SLOT_NEW_LEFT, raw.data(), 1.0f, 0);
      std::vector<float> dIp((size_t)3 * w * h), plane((size_t)w * h);
      dsm_host::check(dsm_tracker_get_frame(trk.handle(), DSM_SLOT_NEW_LEFT, 0, dIp.data()), "dsm_tracker_get_frame");
      for (size_t i = 0; i < plane.size(); i++) plane[i] = dIp[3 * i];
      FILE *f = fopen(argv[3], "wb");
      if (!f || fwrite(plane.data(), sizeof(float), plane.size(), f) != plane.size()) throw std::runtime_error("cannot write the output");
      fclose(f);
      const float *K = und.getK();
      printf("{\"w\": %d, \"h\": %d, \"K\": [%.9g, %.9g, %.9g, %.9g]}\n", w, h, K[0], K[1], K[2], K[3]);
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "%s\n", e.what());
    dsm_context_destroy(ctx);
    return 1;
  }
  dsm_context_destroy(ctx);
  return 0;
}
