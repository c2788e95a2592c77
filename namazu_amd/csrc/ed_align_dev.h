// The banded cell-form edit-distance row step, once: the device pieces that K8 (k_ed_align, ed_align.hip), K8w
// (k_ed_align_wide, ed_align_wide.hip), K11 (pk_lev of k_po_knn, ed_po_knn.hip) and K11w (pkw_lev of k_po_knn_wide,
// ed_po_knn_wide.hip) are built from.
//
// A pair (a, b) of n and m symbols under a band w: row i of the unit-cost matrix D keeps the 2w + 1 cells
// d <-> j = i + d - w. A thread holds C consecutive cells d0 .. d0 + C - 1 in registers (prev[C]: the row above).
// Per 64-row block align_stage puts a[i0 ..] and the block's window of b into LDS; per row
//   1. align_row_candidates: t[d] = min(prev[d] + (a[i-1] != b[j-1]), prev[d + 1] + 1) ("diagonal" and "up"; the
//      thread's last cell takes prev[d + 1] from its neighbour: `nxt`, which the caller fetches), and the thread's
//      running minima lp[c] = min over c' <= c of (t[d'] - d');
//   2. the caller turns the threads' lp[C - 1] into `excl`, the minimum over every thread below (align_scan_min
//      inside a wave; K8w adds the waves below through LDS);
//   3. align_row_close: the horizontal closure D[d] = d + min(excl, lp[c]) into prev[], and whether the thread has a
//      cell <= a threshold (a row without one ends the pair); for a caller that keeps a history (AlignMoves), the 2
//      bits per cell that name the walk's move there -- diag = "the diagonal explains D[d]", low = diag ? "the
//      symbols differ" : "up explains D[d]" -- which the caller ballots into its history.
// align_final_cell picks cell df = m - n + w of the last row out of the owning thread's prev[]. The walk back over
// the move bits is written out in K8 and in K8w (ed_align.hip says why).
// Everything is __forceinline__ over the caller's own registers: no piece owns state, a cross-lane fetch or (apart
// from align_stage) a barrier.
#pragma once
#include "nmz_common.h"

namespace nmz {

constexpr uint32_t ALIGN_ROWS = 64;   // rows per staged block (K8: one history row per lane)
constexpr int32_t ALIGN_INF = 1 << 28;  // beyond any value a live row holds (<= 3 w + 1)

// cells per lane of the one-wave forms (K8, K11) for a band <= 64
inline int align_cells(uint32_t band) { return band <= 31 ? 1 : (band <= 63 ? 2 : 3); }

// The four-wave forms (K8w, K11w): the band's cells blocked over a workgroup of 256 threads, C in {1, 2, 3, 5, 9}
// consecutive cells per thread
constexpr uint32_t AW_THREADS = 256, AW_WAVES = 4;
// the widest band that C cells per thread hold: 2 w + 1 <= 256 C
constexpr int aw_wmax(int C) {
    return ((int)AW_THREADS * C - 1) / 2 < NMZ_ALIGN_WIDE_MAX_BAND ? ((int)AW_THREADS * C - 1) / 2
                                                                   : NMZ_ALIGN_WIDE_MAX_BAND;
}
// cells per thread for a band
__host__ __device__ inline int aw_cells(uint32_t band) {
    const int w = (int)band;
    return w <= aw_wmax(1) ? 1 : (w <= aw_wmax(2) ? 2 : (w <= aw_wmax(3) ? 3 : (w <= aw_wmax(5) ? 5 : 9)));
}
// what a wave tells the others in a row: double-buffered by the row's parity
struct AwRec {
    int32_t wmin;  // min over the wave's cells of t[d] - d
    int32_t t0;    // t of the wave's first cell, -1 if the cell is outside the matrix
    int32_t live;  // the row before had a cell <= the threshold in this wave
    int32_t pad;
};

// Cross-lane moves of the row step as DPP modifiers (data-parallel primitives: no LDS round trip, unlike __shfl).
// A lane without a source -- off the row's end, or in a row the mask leaves out -- keeps `old`.
constexpr int DPP_ROW_SHR = 0x110, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;  // row_shr:n = DPP_ROW_SHR + n
constexpr int DPP_WAVE_SHL1 = 0x130, DPP_WAVE_SHR1 = 0x138;                           // lane i takes lane i + 1 / i - 1
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int32_t align_dpp(int32_t old, int32_t v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xF, false);
}
// inclusive minimum over lanes 0 .. lane: four steps inside each row of 16 lanes, then row 0's last lane into row 1
// and row 2's into row 3, then row 1's last lane into rows 2 and 3
__device__ __forceinline__ int32_t align_scan_min(int32_t v) {
    v = min(v, align_dpp<DPP_ROW_SHR + 1>(ALIGN_INF, v));
    v = min(v, align_dpp<DPP_ROW_SHR + 2>(ALIGN_INF, v));
    v = min(v, align_dpp<DPP_ROW_SHR + 4>(ALIGN_INF, v));
    v = min(v, align_dpp<DPP_ROW_SHR + 8>(ALIGN_INF, v));
    v = min(v, align_dpp<DPP_ROW_BCAST15, 0xA>(ALIGN_INF, v));
    v = min(v, align_dpp<DPP_ROW_BCAST31, 0xC>(ALIGN_INF, v));
    return v;
}

// row 0: D[0][j] = j inside the matrix
template <int C>
__device__ __forceinline__ void align_row0(int32_t (&prev)[C], int32_t d0, int32_t w, int64_t m) {
    const int32_t W2 = 2 * w;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int32_t d = d0 + c;
        const int64_t jv = (int64_t)d - w;
        prev[c] = (d <= W2 && jv >= 0 && jv <= m) ? (int32_t)jv : ALIGN_INF;
    }
}

// The block of rows i0 + 1 .. i0 + 64: s_a[r - 1] = a[i0 + r - 1], s_b[t] = b[i0 - w + t] for t < 64 + 2w, zeros
// outside the traces. Every thread of the workgroup (THREADS of them) calls it, in uniform control flow: the first
// barrier is behind the previous block's reads of s_a / s_b, the second in front of this block's. Stride names the
// type of the window loop's step, which the caller chooses in so many words: int in the one-wave kernels, uint32_t in
// K8w, whose instantiations take more registers than their waves per SIMD allow with a signed step (`make resources`).
template <typename Stride, Stride THREADS>
__device__ __forceinline__ void align_stage(uint64_t *s_a, uint64_t *s_b, const uint64_t *a, int64_t n,
                                            const uint64_t *b, int64_t m, int64_t i0, int32_t w, uint32_t tid) {
    __syncthreads();
    if (THREADS == ALIGN_ROWS || tid < ALIGN_ROWS) s_a[tid] = i0 + tid < n ? a[i0 + tid] : 0;
    for (int32_t t = (int32_t)tid; t < (int32_t)ALIGN_ROWS + 2 * w; t += THREADS) {
        const int64_t jb = i0 - w + t;
        s_b[t] = (jb >= 0 && jb < m) ? b[jb] : 0;
    }
    __syncthreads();
}

// What a kernel that keeps a history takes out of the row step, per cell: the two candidates and whether the symbols
// differ (part 1), then the move bits (part 3). A kernel that wants the distance alone passes AlignNoMoves, and
// nothing of this is worked out.
template <int C>
struct AlignMoves {
    static constexpr bool KEEP = true;
    int32_t dg[C], up[C];
    bool ne[C], diag[C], low[C];
};
struct AlignNoMoves {
    static constexpr bool KEEP = false;
};

// Row i = i0 + r, part 1. nxt: cell d0 + C of the row above.
template <int C, typename Moves>
__device__ __forceinline__ void align_row_candidates(const int32_t (&prev)[C], int32_t nxt, uint64_t ai,
                                                     const uint64_t *s_b, int32_t r, int32_t d0, int32_t w, int64_t m,
                                                     int64_t i, int32_t (&t)[C], bool (&valid)[C], int32_t (&lp)[C],
                                                     Moves &mv) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int32_t d = d0 + c;
        const int64_t jv = i + d - w;
        valid[c] = d <= 2 * w && jv >= 0 && jv <= m;
        const uint64_t bj = s_b[valid[c] ? r + d - 1 : 0];  // b[jv - 1]
        const bool ne = ai != bj;
        const int32_t dg = jv >= 1 ? prev[c] + (ne ? 1 : 0) : ALIGN_INF;
        const int32_t up = (c + 1 < C ? prev[c + 1 < C ? c + 1 : c] : nxt) + 1;
        if constexpr (Moves::KEEP) mv.ne[c] = ne, mv.dg[c] = dg, mv.up[c] = up;
        t[c] = valid[c] ? min(dg, up) : ALIGN_INF;
    }
    // D[d] = d + min over d' <= d of (t[d'] - d')
    lp[0] = t[0] - d0;
#pragma unroll
    for (int c = 1; c < C; ++c) lp[c] = min(lp[c - 1], t[c] - (d0 + c));
}

// Row i, part 3: prev[] becomes row i. excl: the minimum of t[d'] - d' over every cell below d0. Returns whether one
// of the thread's cells is <= thr.
template <int C, typename Moves>
__device__ __forceinline__ bool align_row_close(int32_t (&prev)[C], const bool (&valid)[C], const int32_t (&lp)[C],
                                                int32_t excl, int32_t d0, int32_t thr, Moves &mv) {
    bool live = false;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int32_t cur = valid[c] ? min(d0 + c + min(excl, lp[c]), ALIGN_INF) : ALIGN_INF;
        if constexpr (Moves::KEEP) {
            // diag = valid && dg == cur && cur < INF; low = diag ? ne : (valid && up == cur && cur < INF). Written
            // with & over values read first: as && over mv's arrays the same bits measured 2.7% slower in K8 at C = 2
            // (profiles/align/refactor_ab.json)
            const int32_t dg = mv.dg[c], up = mv.up[c];
            const bool ne = mv.ne[c], reached = valid[c] & (cur < ALIGN_INF);
            const bool diag = reached & (dg == cur), by_up = reached & (up == cur);
            mv.diag[c] = diag;
            mv.low[c] = diag ? ne : by_up;
        }
        live = live || cur <= thr;
        prev[c] = cur;
    }
    return live;
}

// cell df of the last row, in the thread df / C that owns it (the caller fetches it from there)
template <int C>
__device__ __forceinline__ int32_t align_final_cell(const int32_t (&prev)[C], int32_t df) {
    int32_t p[C];  // the values first: a select between loads becomes a load from a selected address, and prev[] a
                   // runtime-indexed array in scratch or LDS
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = prev[c];
    int32_t v = p[0];
#pragma unroll
    for (int c = 1; c < C; ++c) v = (df % C) == c ? p[c] : v;
    return v;
}

}  // namespace nmz
