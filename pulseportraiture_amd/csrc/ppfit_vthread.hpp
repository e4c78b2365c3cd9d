// ppfit_vthread.hpp -- index maps of the one-wave kernels that play a
// 256-thread block (k_post_w beside k_post<false>).  Plain constexpr
// functions of integers, no device code: tools/post_wave_map_check.cpp
// includes this header in a host program and checks the maps exhaustively.
//
// A workgroup of nt threads (nt = 64, or the block itself: nt = block) plays
// the block's threads as "virtual threads": thread tid holds block / nt slots,
// slot q standing for block thread tid + nt q.  Its wave (a "virtual wave") is
// w + (nt / 64) q for real wave w.  Every sum over the block is then formed as
// the block forms it: each virtual thread's terms in its own order, the
// wave's DPP tree per virtual wave, and the virtual waves added in wave order.
#pragma once

#if defined(__HIPCC__)
#define PPF_HD __host__ __device__
#else
#define PPF_HD
#endif

namespace ppf {

// slots per thread of an nt-thread workgroup playing a block of `block`
PPF_HD constexpr int vt_slots(int block, int nt) { return block / nt; }
// the block thread that slot q of thread tid plays
PPF_HD constexpr int vt_thread(int tid, int q, int nt) { return tid + nt * q; }
// the block wave that slot q of real wave w plays
PPF_HD constexpr int vt_wave(int w, int q, int nt) { return w + (nt / 64) * q; }
// Slots that can hold a term when the threads stride over n items (thread t
// takes items t, t + block, ...): slot q's first item is at least nt q.  The
// slots beyond add +0.0 to a sum that started from +0.0 and so is never
// -0.0: leaving them out changes no bit.  At least one slot always runs.
PPF_HD constexpr int vt_live_slots(int n, int block, int nt) {
  const int all = vt_slots(block, nt), need = (n + nt - 1) / nt;
  return need < 1 ? 1 : (need < all ? need : all);
}

// With-scales sweep (sweep<1>): lane (g8, h) of block wave vw takes the
// channels j = 8 gi + g8 of the groups gi = vw, vw + waves, ... and its
// channel lane (h == 0) adds their terms, in that order, into row
// 8 vw + g8 of the block's table; the rows are then added in row order.
PPF_HD constexpr int ws_row(int vw, int g8) { return vw * 8 + g8; }
PPF_HD constexpr int ws_first_group(int vw) { return vw; }
PPF_HD constexpr int ws_chan(int gi, int g8) { return gi * 8 + g8; }
// The row of an nt-thread workgroup's table (8 nt / 64 rows) that holds block
// row ws_row(vt_wave(w, q, nt), g8) while slot q runs: the rows of one slot
// are finished and added, g8 = 0..7 per real wave in wave order, into the
// running totals before the next slot starts -- block row order.
PPF_HD constexpr int ws_local_row(int w, int g8) { return w * 8 + g8; }

}  // namespace ppf
