// post_wave_map_check.cpp -- the index maps of ppfit_vthread.hpp, checked
// exhaustively against the 256-thread block they play, as a stand-alone host
// program (no GPU, no HIP):
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Ipulseportraiture_amd/csrc tools/post_wave_map_check.cpp -o post_wave_map_check
//   ./post_wave_map_check
//
// For every count of fitted channels 1..kMaxChan it walks the loops of
// k_post<false> (block) and of k_post_w (one wave, ppfit_fit.hip) with the same
// helpers the kernels use and compares, operand by operand, what each sum adds
// and in which order.  Exit status 0 and "ok": every map agrees and every row
// index is inside its table.
#include <cstdio>
#include <vector>

#include "ppfit_vthread.hpp"

using namespace ppf;

namespace {

constexpr int kBlock = 256, kWaves = kBlock / 64, kWave = 64;
constexpr int kMaxChan = 80;    // the cases asked for
constexpr int kFarChan = 1100;  // and beyond a block's stride, for the general maps

#define CHECK(cond)                                                               \
  do {                                                                            \
    if (!(cond)) {                                                                \
      fprintf(stderr, "%s:%d: nok %d: %s failed\n", __FILE__, __LINE__, nok, #cond); \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

using Seq = std::vector<int>;

// A block sum: wave v's tree takes lane l's partial, the sum of `items` in
// order; the waves are added in wave order.  part[v][l] = that item list.
using BlockSum = std::vector<std::vector<Seq>>;

// the per-thread channel loops (Sd / fmean, the nu_zero terms, scale errors
// and S/N): for (j = tid; j < nok; j += kBlock)
BlockSum block_thread_sum(int nok) {
  BlockSum p(kWaves, std::vector<Seq>(kWave));
  for (int tid = 0; tid < kBlock; ++tid)
    for (int j = tid; j < nok; j += kBlock) p[tid >> 6][tid & 63].push_back(j);
  return p;
}

int check_thread_sums(int nok) {
  const BlockSum ref = block_thread_sum(nok);
  const int nslot = vt_live_slots(nok, kBlock, kWave);
  CHECK(nslot >= 1 && nslot <= vt_slots(kBlock, kWave));
  CHECK(vt_slots(kBlock, kWave) == kWaves);
  // slot q of the wave is block wave q: the slots run, and are added, in order
  for (int q = 0; q < nslot; ++q) {
    CHECK(vt_wave(0, q, kWave) == q);
    for (int lane = 0; lane < kWave; ++lane) {
      const int vt = vt_thread(lane, q, kWave);
      CHECK(vt >= 0 && vt < kBlock);
      CHECK((vt >> 6) == q && (vt & 63) == lane);  // the same place in the wave's tree
      Seq mine;
      for (int j = vt; j < nok; j += kBlock) mine.push_back(j);
      CHECK(mine == ref[q][lane]);
    }
  }
  // the slots left out hold no term in the block either
  for (int q = nslot; q < kWaves; ++q)
    for (int lane = 0; lane < kWave; ++lane) CHECK(ref[q][lane].empty());
  // nslot = 1 for the block itself: its own threads
  CHECK(vt_live_slots(nok, kBlock, kBlock) == 1 && vt_thread(17, 0, kBlock) == 17);
  return 0;
}

// With-scales sweep.  Block: row 8 w + g8 collects the channels of groups
// gi = w, w + kWaves, ...; rows added in row order.  The result: the rows'
// channel lists in the order the final sum meets them.
std::vector<Seq> block_sweep_rows(int nok) {
  std::vector<Seq> rows(kWaves * 8);
  const int ngroups = (nok + 7) >> 3;
  for (int w = 0; w < kWaves; ++w)
    for (int gi = w; gi < ngroups; gi += kWaves)
      for (int g8 = 0; g8 < 8; ++g8) {
        const int j = gi * 8 + g8;
        if (j < nok) rows[w * 8 + g8].push_back(j);
      }
  return rows;
}

int check_sweep(int nok) {
  const std::vector<Seq> ref = block_sweep_rows(nok);
  const int ngroups = (nok + 7) >> 3;
  const int nslot = vt_live_slots(ngroups, kWaves, 1);
  CHECK(nslot >= 1 && nslot <= kWaves);
  std::vector<Seq> got;  // rows in the order the running total adds them
  for (int sl = 0; sl < nslot; ++sl) {
    const int w = vt_wave(0, sl, kWave);
    CHECK(w == sl);
    std::vector<Seq> lrow(8);  // the wave's table: 8 rows, zeroed per slot
    for (int gi = ws_first_group(w); gi < ngroups; gi += kWaves)
      for (int g8 = 0; g8 < 8; ++g8) {
        const int r = ws_local_row(0, g8);
        CHECK(r >= 0 && r < 8);
        const int j = ws_chan(gi, g8);
        if (j < nok) lrow[r].push_back(j);
      }
    for (int r = 0; r < 8; ++r) {
      CHECK(ws_row(w, r) == (int)got.size());  // block row order
      got.push_back(lrow[r]);
    }
  }
  CHECK(got.size() <= ref.size());
  for (size_t r = 0; r < ref.size(); ++r) {
    if (r < got.size()) CHECK(got[r] == ref[r]);
    else CHECK(ref[r].empty());  // rows of the slots left out: zeros in the block
  }
  // the block's own rows through the same helpers
  for (int w = 0; w < kWaves; ++w)
    for (int g8 = 0; g8 < 8; ++g8) {
      CHECK(ws_row(vt_wave(w, 0, kBlock), g8) == w * 8 + g8);
      CHECK(ws_row(w, g8) < kWaves * 8);
    }
  return 0;
}

}  // namespace

int main() {
  for (int nok = 1; nok <= kFarChan; nok = nok < kMaxChan ? nok + 1 : nok + 37) {
    if (check_thread_sums(nok)) return 1;
    if (check_sweep(nok)) return 1;
  }
  printf("ok\n");
  return 0;
}
