// loop_sequences_demo.cpp -- a node that runs S sequences, each with the loop-closure state of its own LoopHandler (one RingKeyIndex:
// the flann index of LoopHandler.cpp:35-39 and the delay queue of search_place.h:41-56), and searches the ring keys of every
// advance's marginalised keyframes with ONE dsm_host::search_ringkey_many call.  Every call is checked against per-sequence
// search_ringkey calls on twin indexes fed the same keys.  Sequences 0 and 1 see the same places (identical key streams): with one
// index per sequence neither may be handed the other's keyframes.  Every tenth advance sequence 2 marginalises two keyframes.
// Usage: loop_sequences_demo [S] [advances].  Prints one summary line; exit status 0 when every list matched.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "LoopDetection.hpp"

namespace {

struct Rng { // small deterministic generator (no <random> distribution differences between standard libraries)
  unsigned long long s;
  unsigned next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(s >> 33);
  }
};

// ring keys are occupied-sector fractions: multiples of 1/60.  Every fifth keyframe revisits an earlier place (one element moved by
// one sector), the others are new places.
struct Sequence {
  std::unique_ptr<dsm_host::RingKeyIndex> index, twin;
  std::vector<std::vector<float>> keys;
  Rng rng;
  std::vector<float> next_key(int dim) {
    std::vector<float> k(dim);
    if (keys.size() > 20 && keys.size() % 5 == 0) {
      const std::vector<float> &place = keys[rng.next() % (keys.size() - 10)];
      for (int d = 0; d < dim; d++) k[d] = place[d];
      const int d = (int)(rng.next() % dim);
      k[d] = k[d] >= 1.0f ? k[d] - 1.0f / 60 : k[d] + 1.0f / 60;
    } else {
      for (int d = 0; d < dim; d++) k[d] = (float)(rng.next() % 61) / 60.0f;
    }
    keys.push_back(k);
    return k;
  }
};

} // namespace

int main(int argc, char **argv) {
  const int S = argc > 1 ? atoi(argv[1]) : 8, advances = argc > 2 ? atoi(argv[2]) : 260;
  if (S < 3 || advances < 1) {
    fprintf(stderr, "usage: %s [S >= 3] [advances]\n", argv[0]);
    return 2;
  }
  dsm_context *ctx = nullptr;
  if (dsm_context_create(0, &ctx) != DSM_OK) {
    fprintf(stderr, "no device: %s\n", dsm_last_error());
    return 3;
  }
  const int dim = 20;
  long long queries = 0, candidates = 0, mismatches = 0;
  {
    std::vector<Sequence> seqs(S);
    for (int s = 0; s < S; s++) {
      seqs[s].index.reset(new dsm_host::RingKeyIndex(ctx, dim));
      seqs[s].twin.reset(new dsm_host::RingKeyIndex(ctx, dim));
      seqs[s].rng.s = s == 1 ? 1000 : 1000 + (unsigned long long)s; // sequence 1 replays sequence 0's places
    }
    for (int a = 0; a < advances; a++) {
      std::vector<dsm_host::RingKeyIndex *> idx;
      std::vector<std::vector<float>> keys;
      std::vector<int> owner;
      for (int s = 0; s < S; s++) {
        const int n = (s == 2 && a % 10 == 9) ? 2 : 1;
        for (int i = 0; i < n; i++) {
          idx.push_back(seqs[s].index.get());
          keys.push_back(seqs[s].next_key(dim));
          owner.push_back(s);
        }
      }
      std::vector<const float *> kp;
      for (auto &k : keys) kp.push_back(k.data());
      std::vector<std::vector<int>> got;
      dsm_host::search_ringkey_many(idx, kp, got);
      for (size_t j = 0; j < keys.size(); j++) {
        std::vector<int> want;
        seqs[owner[j]].twin->search_ringkey(keys[j].data(), want);
        queries++;
        candidates += (long long)got[j].size();
        if (got[j] != want) {
          if (mismatches < 5) fprintf(stderr, "advance %d, sequence %d: %zu candidates, %zu sequential\n", a, owner[j], got[j].size(), want.size());
          mismatches++;
        }
      }
    }
    for (int s = 0; s < S; s++)
      if (seqs[s].index->size() != seqs[s].twin->size()) mismatches++;
  }
  dsm_context_destroy(ctx);
  printf("loop_sequences_demo: sequences=%d advances=%d queries=%lld candidates=%lld mismatches=%lld\n", S, advances, queries, candidates,
         mismatches);
  return mismatches == 0 && candidates > 0 ? 0 : 1;
}
