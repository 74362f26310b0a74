// pose_batch_demo.cpp -- the loop chain of a node that serves S sequences, through the C++ adaptors, with every batched step taken once
// for all sequences: ScanContext::generate of each sequence's current keyframe, ONE search_ringkey_many over the sequences' own
// indexes, search_sc against the candidates' signatures, ONE PoseEstimatorBatch::estimate over the matches (LoopHandler.cpp:274-279), and
// ONE icp_many over the matches direct alignment rejected (:284-288).
// Input file (native byte order): int32 S, w, h, levels; double lidar_range; then per sequence
//   float cam[4]; double guess[16] (row-major tfm of the matched keyframe in the current one);
//   int32 n_hist, and per earlier keyframe: int32 n_sph, n_sph x 3 doubles (pts_spherical); int32 n_pts, n_pts x 3 doubles (pts_dso xyz),
//     levels x n_pts floats (their colours per level); float ab_exposure
//   the current keyframe: int32 n_sph, n_sph x 3 doubles; levels pyramids of w_l x h_l (I, dx, dy) floats; float ab_exposure
// The earlier keyframes' ring keys are put into the index directly (they are past the LOOP_MARGIN delay).
// Usage: pose_batch_demo FILE.  Prints one JSON line per sequence.
#include <cstdio>
#include <memory>
#include <vector>

#include "LoopDetection.hpp"
#include "TrackerAndScaler.hpp"

namespace {

struct Keyframe {
  std::vector<double> sph, xyz;
  std::vector<std::vector<float>> colors;
  std::vector<const float *> color_ptrs;
  float ab_exposure = 1.0f;
  dsm_host::SigType signature;
};
struct Sequence {
  float cam[4];
  double guess[16];
  std::vector<Keyframe> hist;
  std::vector<double> cur_sph;
  std::vector<std::vector<float>> cur_pyr;
  std::vector<const float *> cur_ptrs;
  float cur_exposure = 1.0f;
  std::unique_ptr<dsm_host::RingKeyIndex> index;
  std::vector<float> ringkey;
  dsm_host::SigType signature;
  std::vector<int> candidates;
  int matched = -1;
  float sc_diff = 0.f;
};

template <typename T>
bool get(FILE *f, T *p, size_t n = 1) { return fread(p, sizeof(T), n, f) == n; }
template <typename T>
bool get_vec(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || get(f, v.data(), n);
}

} // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: pose_batch_demo FILE\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int S = 0, w = 0, h = 0, levels = 0;
  double lidar_range = 0;
  if (!f || !get(f, &S) || !get(f, &w) || !get(f, &h) || !get(f, &levels) || !get(f, &lidar_range) || S < 1 || levels < 1 || levels > DSM_MAX_LEVELS) {
    fprintf(stderr, "pose_batch_demo: cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<Sequence> seqs(S);
  bool good = true;
  for (Sequence &q : seqs) {
    int n_hist = 0, n = 0;
    good = good && get(f, q.cam, 4) && get(f, q.guess, 16) && get(f, &n_hist) && n_hist >= 0;
    if (!good) break;
    q.hist.resize(n_hist);
    for (Keyframe &k : q.hist) {
      good = good && get(f, &n) && n >= 0 && get_vec(f, k.sph, (size_t)3 * n);
      good = good && get(f, &n) && n >= 0 && get_vec(f, k.xyz, (size_t)3 * n);
      k.colors.resize(levels);
      for (int l = 0; l < levels && good; l++) good = get_vec(f, k.colors[l], (size_t)n);
      good = good && get(f, &k.ab_exposure);
      for (int l = 0; l < levels; l++) k.color_ptrs.push_back(k.colors[l].data());
    }
    good = good && get(f, &n) && n >= 0 && get_vec(f, q.cur_sph, (size_t)3 * n);
    q.cur_pyr.resize(levels);
    for (int l = 0; l < levels && good; l++) good = get_vec(f, q.cur_pyr[l], (size_t)3 * (w >> l) * (h >> l));
    good = good && get(f, &q.cur_exposure);
    for (int l = 0; l < levels; l++) q.cur_ptrs.push_back(q.cur_pyr[l].data());
  }
  fclose(f);
  if (!good) {
    fprintf(stderr, "pose_batch_demo: short file\n");
    return 2;
  }
  dsm_context *ctx = nullptr;
  dsm_host::loop_check(dsm_context_create(0, &ctx), "dsm_context_create");
  int rc = 0;
  try {
    const dsm_host::ScanContext sc;
    double tfm_pca_rig[16];
    // every sequence's index holds its earlier keyframes; the current keyframes' descriptors
    std::vector<dsm_host::RingKeyIndex *> indexes;
    std::vector<const float *> keys;
    for (Sequence &q : seqs) {
      q.index.reset(new dsm_host::RingKeyIndex(ctx, (int)sc.getHeight()));
      for (Keyframe &k : q.hist) {
        std::vector<float> key;
        sc.generate(k.sph, key, k.signature, lidar_range, tfm_pca_rig);
        dsm_host::loop_check(dsm_ringdb_add_points(q.index->handle(), key.data(), 1), "dsm_ringdb_add_points");
      }
      sc.generate(q.cur_sph, q.ringkey, q.signature, lidar_range, tfm_pca_rig);
      indexes.push_back(q.index.get());
      keys.push_back(q.ringkey.data());
    }
    // detect: one call for all sequences, then search_sc per sequence (at most FLANN_NN candidates each)
    std::vector<std::vector<int>> cands;
    dsm_host::search_ringkey_many(indexes, keys, cands);
    std::vector<dsm_host::PoseMatch> matches;
    std::vector<int> seq_of;
    for (int s = 0; s < S; s++) {
      Sequence &q = seqs[s];
      q.candidates = cands[s];
      if (q.candidates.empty()) continue;
      dsm_host::search_sc(q.signature, [&q](int i) -> const dsm_host::SigType & { return q.hist[i].signature; }, q.candidates, (int)sc.getWidth(),
                          q.matched, q.sc_diff);
      const Keyframe &k = q.hist[q.matched];
      dsm_host::PoseMatch m;
      m.n = (int)(k.xyz.size() / 3), m.xyz = k.xyz.data(), m.ref_colors = k.color_ptrs.data(), m.ref_ab_exposure = k.ab_exposure;
      m.new_fh.dIp = q.cur_ptrs.data(), m.new_fh.ab_exposure = q.cur_exposure;
      for (int c = 0; c < 4; c++) m.new_cam[c] = q.cam[c];
      for (int e = 0; e < 16; e++) m.ref_to_new[e] = q.guess[e];
      matches.push_back(m);
      seq_of.push_back(s);
    }
    // direct alignment of every match in one call; the ICP fallback of the rejected ones in one call
    dsm_host::PoseEstimatorBatch estimator(ctx, w, h, levels);
    estimator.estimate(matches, levels - 1);
    std::vector<dsm_host::IcpMatch> fallback;
    std::vector<int> fallback_of(matches.size(), -1);
    for (size_t j = 0; j < matches.size(); j++) {
      if (matches[j].ok) continue;
      const Sequence &q = seqs[seq_of[j]];
      dsm_host::IcpMatch im;
      im.pts_source = &q.hist[q.matched].sph, im.pts_target = &q.cur_sph;
      for (int e = 0; e < 16; e++) im.tfm_target_source[e] = q.guess[e];
      fallback_of[j] = (int)fallback.size();
      fallback.push_back(im);
    }
    dsm_host::icp_many(ctx, fallback);
    std::vector<int> match_of(S, -1);
    for (size_t j = 0; j < matches.size(); j++) match_of[seq_of[j]] = (int)j;
    for (int s = 0; s < S; s++) {
      const Sequence &q = seqs[s];
      printf("{\"seq\": %d, \"candidates\": [", s);
      for (size_t c = 0; c < q.candidates.size(); c++) printf("%s%d", c ? ", " : "", q.candidates[c]);
      printf("], \"matched\": %d", q.matched);
      if (match_of[s] >= 0) {
        const dsm_host::PoseMatch &m = matches[match_of[s]];
        printf(", \"sc_diff\": %.9g, \"ok\": %d, \"pose_error\": %.9g, \"inlier_percent\": %d, \"ref_to_new\": [", (double)q.sc_diff, (int)m.ok,
               (double)m.pose_error, m.inlier_percent);
        for (int e = 0; e < 16; e++) printf("%s%.17g", e ? ", " : "", m.ref_to_new[e]);
        printf("]");
        const int fb = fallback_of[match_of[s]];
        if (fb >= 0) {
          printf(", \"icp_ok\": %d, \"icp_score\": %.9g, \"icp_tfm\": [", (int)fallback[fb].ok, (double)fallback[fb].icp_score);
          for (int e = 0; e < 16; e++) printf("%s%.17g", e ? ", " : "", fallback[fb].tfm_target_source[e]);
          printf("]");
        }
      }
      printf("}\n");
    }
  } catch (const std::exception &e) {
    fprintf(stderr, "pose_batch_demo: %s\n", e.what());
    rc = 1;
  }
  for (Sequence &q : seqs) q.index.reset(); // the indexes go before their context
  dsm_context_destroy(ctx);
  return rc;
}
