// sample_common.hpp -- what sph_sample (sample.hip) and sph_trace (trace.hip) share: the device-side view of the level / cell
// search structure over the sources, the per-point walk over it, and the host-side entry that builds it.
//
// The structure is a function of the source set and the descriptor only (include/summersph.h, sph_sample, "Order"), and
// point_sums adds a point's sources in one documented order.  Both passes therefore give a point the same bits.
//
// Include this after `#pragma clang fp contract(off)`: the per-pair arithmetic must not contract into fused multiply-adds.
#pragma once
#include "cell_table.hpp"

namespace sph {

constexpr int SAMPLE_HBINS = 8192;         // quarter octaves of a positive double: bits >> 50
constexpr double SAMPLE_DBL_BIG = 1.7976931348623157e308;
constexpr uint64_t POINT_KEY_NONE = (uint64_t)1 << (3 * LEVEL_AXIS_BITS);     // a point without a cell: sorts last

struct Level {
    double edge, inv_e;                    // cell edge E_l and 1 / E_l
    double cull2;                          // (2 H_l)^2 (1 + 1e-5): a cell farther than this (squared) holds no reaching source
    int32_t cmax[3];                       // largest cell index per axis
    int32_t pad;
};

// on the device, written by sample_levels (counts by sample_walk)
struct Info {
    double lo[3];                          // the source box's minimum: origin of every level's cells
    int64_t n_src;                         // sources (sorted positions [0, n_src))
    int64_t counts[2];                     // points with den != 0 (-1: a source has a bad h), points with a non-finite coordinate
    int32_t bad;
    int32_t nlev;                          // occupied levels
    int32_t top;                           // the most populated level (the points are sorted by their cell in it)
    int32_t g;                             // a level is an aligned group of 2^g quarter octaves
    Level lv[MAX_LEVELS];
    uint8_t level_of[SAMPLE_HBINS];        // quarter octave -> level
};

// the structure as a walk reads it: all device memory inside the analysis scratch, valid until the next analysis call
struct SampleView {
    Info *info;
    const double4 *rec;                    // {x, y, z, 1 / h} in (level, cell, id) order
    const double *wsa;                     // {ws, ws A^(0..nf-1)} per record, stride nf + 1
    const Ent *tab;                        // (level, cell) -> [start, end)
    uint64_t mask;
};

// what sample_build needs of a call
struct SampleSources {
    const double *clip_lo, *clip_hi;       // the strict source clip box
    double h_one;                          // > 0: h of every source; 0: SPH_F_H (per_h)
    bool per_h, volume, host;
    int nf;                                // rows of wsa beyond ws
    const int32_t *fields;                 // nf ids: SPH_F_* or -1 (row k of values)
    const double *values;                  // host (host form) or device memory, or null
    size_t tmp_bytes;                      // the caller's own need of sort_tmp
};

// Builds the structure on c->stream: select -> levels -> keys -> sort -> records -> tails.  One scratch allocation holds
// the structure, `extra_bytes` for the caller (returned 256-byte aligned in *extra; carve it with Carve{*extra}) and a sort
// workspace of max(own, tmp_bytes) in *sort_tmp.  A host form's VALUES rows are copied to the device here.
int sample_build(sph_ctx *c, const SampleSources &src, size_t extra_bytes, SampleView *view, char **extra, char **sort_tmp);

__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return fabs(x) <= SAMPLE_DBL_BIG && fabs(y) <= SAMPLE_DBL_BIG && fabs(z) <= SAMPLE_DBL_BIG;
}

// render.hip's kernel_w: 1 - 1.5 q^2 + 0.75 q^3 (q <= 1), 0.25 (2 - q)^3 (1 < q <= 2), 0 beyond
__device__ __forceinline__ double kernel_w(double q) {
    const double t = 2.0 - q;
    const double w1 = (1.0 - 1.5 * (q * q)) + 0.75 * (q * q * q);
    const double w2 = 0.25 * (t * t * t);
    return q <= 1.0 ? w1 : (q <= 2.0 ? w2 : 0.0);
}

// a point's sort key: its (clamped) cell in the most populated level, POINT_KEY_NONE for a non-finite point
__device__ __forceinline__ uint64_t point_sort_key(const Info *__restrict__ info, double x, double y, double z) {
    if (!finite3(x, y, z)) return POINT_KEY_NONE;
    if (info->nlev <= 0) return 0;
    const Level &L = info->lv[info->top];
    return level_key(0, level_cell_axis(x, info->lo[0], L.inv_e, L.cmax[0]), level_cell_axis(y, info->lo[1], L.inv_e, L.cmax[1]),
                     level_cell_axis(z, info->lo[2], L.inv_e, L.cmax[2]));
}

// the sources at sorted positions [q0, q1) added to a point's sums, in that order
template <int K, bool PER_H>
__device__ __forceinline__ void add_range(const double4 *__restrict__ rec, const double *__restrict__ wsa, int32_t q0, int32_t q1,
                                          const double (&p)[3], double ih_one, double &den, double (&num)[K > 0 ? K : 1]) {
    constexpr int S = K + 1;
    for (int32_t q = q0; q < q1; q++) {
        const double4 s = rec[q];
        const double dx = p[0] - s.x, dy = p[1] - s.y, dz = p[2] - s.z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const double ih = PER_H ? s.w : ih_one;
        if (!(d2 * (ih * ih) <= 4.0000001)) continue;      // filter only: q <= 2 decides
        const double qq = sqrt(d2) * ih;
        if (!(qq <= 2.0)) continue;
        const double wn = kernel_w(qq);
        const double *w = wsa + (int64_t)q * S;
        den += w[0] * wn;
#pragma unroll
        for (int k = 0; k < K; k++) num[k] += w[1 + k] * wn;
    }
}

// den and num[K] of the point p added up over the first nlev levels (the caller's zeros on entry): the levels in ascending
// order, in each the <= 27 cells around the point's (signed, unclamped) cell that lie inside the source box, in ascending
// key, skipping a cell whose nearest face is farther than 2 H_l; each cell's records in id order
template <int K, bool PER_H>
__device__ __forceinline__ void point_sums(const Info *__restrict__ info, const double4 *__restrict__ rec,
                                           const double *__restrict__ wsa, const Ent *__restrict__ tab, uint64_t mask, int nlev,
                                           const double (&p)[3], double ih_one, double &den, double (&num)[K > 0 ? K : 1]) {
    for (int l = 0; l < nlev; l++) {
        const Level &L = info->lv[l];
        const double e = L.edge, cull2 = L.cull2;
        // the stencil: the signed, unclamped cell of the point +- 1, intersected with the source box's cells
        int32_t c0[3], c1[3];
        bool any = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double cm = (double)L.cmax[a];
            const double fc = fmin(fmax(floor((p[a] - info->lo[a]) * L.inv_e), -2.0), cm + 2.0);
            const int32_t ci = (int32_t)fc;
            c0[a] = max(ci - 1, 0);
            c1[a] = min(ci + 1, L.cmax[a]);
            any = any && c0[a] <= c1[a];
        }
        if (!any) continue;
        for (int32_t n0 = c0[0]; n0 <= c1[0]; n0++) {
            const double f0 = info->lo[0] + (double)n0 * e;
            const double g0 = fmax(fmax(f0 - p[0], p[0] - (f0 + e)), 0.0);
            for (int32_t n1 = c0[1]; n1 <= c1[1]; n1++) {
                const double f1 = info->lo[1] + (double)n1 * e;
                const double g1 = fmax(fmax(f1 - p[1], p[1] - (f1 + e)), 0.0);
                const double g01 = g0 * g0 + g1 * g1;
                if (g01 > cull2) continue;
                for (int32_t n2 = c0[2]; n2 <= c1[2]; n2++) {
                    const double f2 = info->lo[2] + (double)n2 * e;
                    const double g2 = fmax(fmax(f2 - p[2], p[2] - (f2 + e)), 0.0);
                    if (g01 + g2 * g2 > cull2) continue;     // no source of this level in the cell reaches the point
                    const int64_t en = hash_slot(tab, mask, level_key((uint64_t)l, (uint64_t)n0, (uint64_t)n1, (uint64_t)n2));
                    if (en < 0) continue;
                    add_range<K, PER_H>(rec, wsa, tab[en].start, tab[en].end, p, ih_one, den, num);
                }
            }
        }
    }
}

}  // namespace sph
