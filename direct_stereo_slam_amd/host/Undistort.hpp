// Undistort.hpp -- C++ host adaptor with the surface of UPSTREAM-DSO's dso::Undistort as the reference node uses it
// (main.cpp:246-256: undistorterN_->undistort<unsigned char>(&img, 1, 0, 1.0f), then getK() for makeK, main.cpp:237),
// on top of the C ABI: the remap is built once on the host (dsm_pinhole_undistort_map), photometric correction and remap run
// on the device at the hand-over (dsm_upload_images_undistorted).  Header-only, plain C++11; Pinhole camera files only
// (other models: build the table yourself and use the table constructor).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsm_hotpath.h"
#include "TrackerAndScaler.hpp"

namespace dsm_host {

// DSO's four-line camera file: `Pinhole fx fy cx cy 0` / `W H` / `crop | none | fx fy cx cy 0` / `W' H'`
struct CameraFile {
  double calib[4] = {0, 0, 0, 0};
  int w_in = 0, h_in = 0;
  int out_mode = DSM_UNDISTORT_CROP;
  float out_calib[4] = {0, 0, 0, 0};
  int w_out = 0, h_out = 0;
};
inline CameraFile readCameraFile(const std::string &path) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error("readCameraFile: cannot open " + path);
  std::string l1, l2, l3, l4;
  if (!std::getline(f, l1) || !std::getline(f, l2) || !std::getline(f, l3) || !std::getline(f, l4))
    throw std::runtime_error(path + ": a camera file has four lines");
  CameraFile c;
  std::istringstream s1(l1);
  std::string model;
  s1 >> model >> c.calib[0] >> c.calib[1] >> c.calib[2] >> c.calib[3];
  if (!s1 || model != "Pinhole") throw std::runtime_error(path + ": line 1 is not `Pinhole fx fy cx cy 0`");
  std::istringstream s2(l2);
  if (!(s2 >> c.w_in >> c.h_in)) throw std::runtime_error(path + ": line 2 is not `W H`");
  std::istringstream s3(l3);
  std::string word;
  s3 >> word;
  if (word == "crop") {
    c.out_mode = DSM_UNDISTORT_CROP;
  } else if (word == "none") {
    c.out_mode = DSM_UNDISTORT_NONE;
  } else {
    float v[5];
    // (read with %f upstream)
    if (std::sscanf(l3.c_str(), "%f %f %f %f %f", &v[0], &v[1], &v[2], &v[3], &v[4]) != 5)
      throw std::runtime_error(path + ": line 3 is `crop`, `none` or five numbers (`full` is not supported)");
    c.out_mode = DSM_UNDISTORT_EXPLICIT;
    for (int k = 0; k < 4; k++) c.out_calib[k] = v[k];
  }
  std::istringstream s4(l4);
  if (!(s4 >> c.w_out >> c.h_out)) throw std::runtime_error(path + ": line 4 is not `W' H'`");
  return c;
}

class Undistort {
public:
  // dso::Undistort::getUndistorterForFile(configFilename, gammaFilename, vignetteFilename) with the photometric tables
  // already decoded: G = 256 floats (rescaled response) or null, vignette_inv = w_in * h_in floats or null.  w_out, h_out
  // > 0 override the file's fourth line (benchmarkSetting_width / height, main.cpp:110-111).
  Undistort(dsm_context *ctx, const std::string &camera_file, const float *G = nullptr, const float *vignette_inv = nullptr, int w_out = 0,
            int h_out = 0) {
    check_abi();
    const CameraFile c = readCameraFile(camera_file);
    w_in_ = c.w_in, h_in_ = c.h_in;
    w_ = w_out > 0 ? w_out : c.w_out;
    h_ = h_out > 0 ? h_out : c.h_out;
    std::vector<float> rx((size_t)w_ * h_), ry((size_t)w_ * h_);
    int passthrough = 0;
    check(dsm_pinhole_undistort_map(c.calib, w_in_, h_in_, c.out_mode, c.out_calib, w_, h_, K_, &passthrough, rx.data(), ry.data()),
          "dsm_pinhole_undistort_map");
    create(ctx, passthrough ? nullptr : rx.data(), passthrough ? nullptr : ry.data(), G, vignette_inv);
  }
  // a caller's table (any camera model): remap_x / remap_y w_out * h_out source coordinates (-1 = outside), K = the output camera
  Undistort(dsm_context *ctx, int w_in, int h_in, int w_out, int h_out, const float *remap_x, const float *remap_y, const float K[4],
            const float *G = nullptr, const float *vignette_inv = nullptr)
      : w_(w_out), h_(h_out), w_in_(w_in), h_in_(h_in) {
    check_abi();
    for (int k = 0; k < 4; k++) K_[k] = K[k];
    create(ctx, remap_x, remap_y, G, vignette_inv);
  }
  ~Undistort() { dsm_undistorter_destroy(u_); }
  Undistort(const Undistort &) = delete;
  Undistort &operator=(const Undistort &) = delete;

  // getK(): fx, fy, cx, cy of the output camera -- what makeK and the FrontEnd constructor take (main.cpp:237)
  const float *getK() const { return K_; }
  void getSize(int &w, int &h) const { w = w_, h = h_; }
  void getOriginalSize(int &w, int &h) const { w = w_in_, h = h_in_; }
  const dsm_undistorter *handle() const { return u_; }

  // undistort<unsigned char>(img, 1, 0, 1.0f) + the hand-over of its result to `slot` of `tracker`, in one call: the pyramid is
  // built on the device and the slot counts as holding `unique_id` afterwards (as TrackerAndScaler::uploadImage)
  void uploadImage(TrackerAndScaler &tracker, int slot, const uint8_t *pixels, float ab_exposure, long long unique_id,
                   size_t row_pitch_bytes = 0) const {
    dsm_tracker *ts[1] = {tracker.handle()};
    const int slots[1] = {slot};
    const void *imgs[1] = {pixels};
    const float ex[1] = {ab_exposure};
    check(dsm_upload_images_undistorted(ctx_, u_, 1, ts, slots, imgs, ex, row_pitch_bytes, DSM_UPLOAD_SYNC), "Undistort::uploadImage");
    tracker.noteResident(slot, unique_id);
  }

private:
  void create(dsm_context *ctx, const float *rx, const float *ry, const float *G, const float *vig) {
    ctx_ = ctx;
    check(dsm_undistorter_create(ctx, w_in_, h_in_, w_, h_, rx, ry, G, vig, &u_), "dsm_undistorter_create");
  }
  dsm_context *ctx_ = nullptr;
  dsm_undistorter *u_ = nullptr;
  float K_[4] = {0, 0, 0, 0};
  int w_ = 0, h_ = 0, w_in_ = 0, h_in_ = 0;
};

// Undistort::uploadImage for many trackers in ONE hand-over (the raw camera bytes of both cameras of several sequences arrive
// together); form: DSM_UPLOAD_SYNC / DSM_UPLOAD_ASYNC (slots DSM_SLOT_NEXT_*, then dsm_frames_advance) / DSM_UPLOAD_ENQUEUE
inline void uploadImagesUndistorted(dsm_context *ctx, const Undistort &und, const std::vector<TrackerAndScaler *> &trackers,
                                    const std::vector<int> &slots, const std::vector<const void *> &pixels,
                                    const std::vector<float> &ab_exposures, const std::vector<long long> &unique_ids,
                                    size_t row_pitch_bytes = 0, int form = DSM_UPLOAD_SYNC) {
  const size_t n = trackers.size();
  if (!n) return;
  if (slots.size() != n || pixels.size() != n || ab_exposures.size() != n || unique_ids.size() != n)
    throw std::runtime_error("uploadImagesUndistorted: sizes differ");
  std::vector<dsm_tracker *> ts(n);
  for (size_t i = 0; i < n; i++) ts[i] = trackers[i]->handle();
  check(dsm_upload_images_undistorted(ctx, und.handle(), (int)n, ts.data(), slots.data(), pixels.data(), ab_exposures.data(), row_pitch_bytes,
                                      form),
        "uploadImagesUndistorted");
  for (size_t i = 0; i < n; i++) // (back buffers, DSM_SLOT_NEXT_*: resident once dsm_frames_advance swapped them in)
    if (slots[i] < 2) trackers[i]->noteResident(slots[i], unique_ids[i]);
}

} // namespace dsm_host
