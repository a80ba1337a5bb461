// The flush coefficients of the per-K GEMM family — ONE statement of the formula, for the device (every kernel's prologue stages its
// table through it, gemm_tile.h) and for a plain C++ compiler (tests/host/flush_coef_main.cpp checks it on a CPU against
// dgq_amd/plan.py:flush_coefficients).  This header includes nothing.
//
// Summation by parts: with T the RUNNING int32 total of a chunk sequence and δ_c the scale of chunk c's group,
// Σ_groups δ_g·P_g = Σ_c (δ_c − δ_next(c))·T_c, δ := 0 past the sequence.  The coefficient is non-zero exactly at group ends, so a flush
// is cvt + fma per accumulator register.  A kernel runs several sequences: consecutive chunks of one sequence are S chunks apart in
// the linear chunk order (S = accumulator sets x K waves inside a tile: ACCS·WVK in the tile kernel, ACCS in the panel / convq kernels,
// 1 in the 256-row kernel and in plan.flush_coefficients), and a sequence ends with the K range that owns it (the K slice of the
// workgroup; in the panel kernel the per_kw tiles of one K wave).  A clear mark (cflush == 2) on the LAST chunk of a K tile asks for
// the totals to be cleared behind that tile (|T| < 2^24: float(T) exact, dgq_amd/plan.py:mark_clears): the coefficient of each
// sequence's last chunk in the tile is then the full δ_c.  Marks on other chunks are not honoured (the planner places none).
#pragma once

#if defined(__HIP__)
#define DGQ_FLUSH_FN __host__ __device__ inline
#else
#define DGQ_FLUSH_FN inline
#endif

#define NCH 4                 // 32-wide chunks per K tile

struct FlushGeom {
    int S;                    // distance between consecutive chunks of one running-total sequence
    int kt_begin, nk;         // the K slice: K tiles [kt_begin, kt_begin + nk) of the problem's nk_total
    int nk_total;
    int per_kw;               // slice tiles per K range; 0: the slice is one range
};

// What one table entry reads (cdelta[g], cdelta[gn], cflush[tl]) and how it combines them: the coefficient of chunk g, or the clear
// flag of a slice tile.
struct FlushRef {
    int g, gn, tl;
    bool is_coef, tile_end, seq_last, not_last;
};

DGQ_FLUSH_FN int flush_range_last(const FlushGeom& q, int t) {          // last slice tile of the K range that owns slice tile t
    if (q.per_kw <= 0) return q.nk - 1;
    const int e = (t / q.per_kw + 1) * q.per_kw;
    return (e < q.nk ? e : q.nk) - 1;
}

// Entry of chunk g (is_coef; g: linear chunk index of the whole problem) or of slice tile t (!is_coef; g: any chunk of the problem,
// read and ignored).  Branch-free: a kernel's threads take both kinds side by side.
DGQ_FLUSH_FN FlushRef flush_ref(const FlushGeom& q, bool is_coef, int g, int t) {
    FlushRef x;
    const int tg = g / NCH, c = g - tg * NCH, last = q.nk_total * NCH - 1;
    t = is_coef ? tg - q.kt_begin : t;
    const int range_last = flush_range_last(q, t);
    x.is_coef = is_coef;
    x.g = g;
    x.gn = g + q.S < last ? g + q.S : last;
    x.tl = (q.kt_begin + t) * NCH + NCH - 1;
    x.tile_end = c + q.S >= NCH;                                        // last chunk of its sequence in the tile
    x.seq_last = x.tile_end && t == range_last;
    x.not_last = t != range_last;                                       // no clear behind the last tile of a range
    return x;
}
DGQ_FLUSH_FN FlushRef flush_ref_coef(const FlushGeom& q, int g) { return flush_ref(q, true, g, 0); }
DGQ_FLUSH_FN FlushRef flush_ref_flag(const FlushGeom& q, int t) { return flush_ref(q, false, q.kt_begin * NCH, t); }

DGQ_FLUSH_FN float flush_value(const FlushRef& x, float d, float dn, unsigned cf) {
    const bool clr = (cf & 0xFF) == 2;
    const float coef = (x.seq_last || (x.tile_end && clr)) ? d : d - dn;
    const float flag = (x.not_last && clr) ? 1.0f : 0.0f;
    return x.is_coef ? coef : flag;
}

DGQ_FLUSH_FN float flush_entry(const FlushRef& x, const float* cdelta, const unsigned char* cflush) {
    return flush_value(x, cdelta[x.g], cdelta[x.gn], cflush[x.tl]);
}
