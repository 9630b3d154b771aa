// image_common.hpp -- what the image passes (render.hip, cube.hip, transfer.hip, frames.hip) define in common: which
// particles a call selects and with which h, how far a particle reaches, where the np.linspace nodes sit and which of them
// lie within a reach (node_range: transfer.hip's tiles, frames.hip's footprints), the viewing frame, the start table of a
// sorted key array and the host checks that go with them.  The order-rule and determinism tests and the
// comparison of sph_transfer against sph_cube rely on these being one function in every pass.  The binning itself
// (3-D cells, image-plane cells, depth-sorted tile lists) differs per pass and stays in its file.
#pragma once
#include <cmath>
#include <string>

#include "reduce_common.hpp"

// the definitions fix the order of every sum; no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

struct Sel {
    double clip_lo[3], clip_hi[3];
    double h;                      // > 0: one h for every particle; else per particle from hf
    const double *hf;
    const int32_t *orig;
    int64_t n_slots;
    int32_t n_owned;
};

__device__ __forceinline__ bool selected(const Sel &s, int64_t i, double px, double py, double pz) {
    return s.orig[i] < s.n_owned && px > s.clip_lo[0] && px < s.clip_hi[0] && py > s.clip_lo[1] && py < s.clip_hi[1] &&
           pz > s.clip_lo[2] && pz < s.clip_hi[2];
}

// the h of slot i
__device__ __forceinline__ double sel_h(const Sel &s, int64_t i) { return s.h > 0.0 ? s.h : s.hf[i]; }

// how far a particle of smoothing length h reaches: 2 h and a margin for the rounding of the node coordinates
__host__ __device__ __forceinline__ double reach_of(double h) { return 2.0 * h * (1.0 + 1e-6); }
__device__ __forceinline__ double sel_reach(const Sel &s, int64_t i) { return reach_of(sel_h(s, i)); }

template <int D>
struct Nodes {
    double lo[D], hi[D], step[D];  // hi = lo where n == 1
    int32_t n[D];
};

// np.linspace: i * step + lo, the last node exactly hi
template <int D>
__device__ __forceinline__ double node_coord(const Nodes<D> &nd, int a, int i) {
    return i >= nd.n[a] - 1 ? nd.hi[a] : (double)i * nd.step[a] + nd.lo[a];
}

// the nodes i0 .. i1 of axis a with p - reach <= node <= p + reach, decided on the node coordinates themselves (the
// division only gives the first guess); false when there is none (or p is NaN)
__device__ __forceinline__ bool node_range(const Nodes<2> &nd, int a, double p, double reach, int &i0, int &i1) {
    const double a0 = p - reach, a1 = p + reach;
    const int n = nd.n[a];
    if (!(a1 >= nd.lo[a] && a0 <= nd.hi[a])) return false;
    i0 = 0;
    i1 = n - 1;
    if (n == 1 || !(nd.step[a] > 0.0) || !(nd.step[a] < INFINITY)) return true;     // every node sits on lo (or the step overflowed)
    const double last = (double)(n - 1);
    i0 = (int)fmin(fmax(ceil((a0 - nd.lo[a]) / nd.step[a]), 0.0), last);
    i1 = (int)fmin(fmax(floor((a1 - nd.lo[a]) / nd.step[a]), 0.0), last);
    while (i0 > 0 && node_coord(nd, a, i0 - 1) >= a0) i0--;
    while (node_coord(nd, a, i0) < a0) i0++;               // stops at n - 1 at the latest: hi >= a0
    while (i1 < n - 1 && node_coord(nd, a, i1 + 1) <= a1) i1++;
    while (node_coord(nd, a, i1) > a1) i1--;               // stops at 0 at the latest: lo <= a1
    return i0 <= i1;
}

struct Frame {
    double rot[9], centre[3];      // rows u^, v^, w^; P = rot (r - centre)
};

// row a of rot applied to d, in the definition's order
__device__ __forceinline__ double row_dot(const double *r, int a, double dx, double dy, double dz) {
    return (r[3 * a] * dx + r[3 * a + 1] * dy) + r[3 * a + 2] * dz;
}

// start[c] = first of the n sorted keys whose high word is >= c (c in [0, ncells]): a cell's or a tile's first record
static __global__ __launch_bounds__(256) void start_table(const uint64_t *__restrict__ keys, int64_t n, int64_t ncells,
                                                          int32_t *__restrict__ start) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > ncells) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)(keys[mid] >> 32) < c) lo = mid + 1; else hi = mid;
    }
    start[c] = (int32_t)lo;
}

// ---- host ---------------------------------------------------------------------------------------------------------------

// h: the descriptor's (0: the context's own, per particle where it is variable)
inline Sel make_sel(const sph_ctx *c, const double *clip_lo, const double *clip_hi, double h) {
    Sel s{};
    for (int a = 0; a < 3; a++) { s.clip_lo[a] = clip_lo[a]; s.clip_hi[a] = clip_hi[a]; }
    s.h = h > 0.0 ? h : (c->variable ? 0.0 : c->p.h);
    s.hf = c->variable ? c->f[SPH_F_H] : nullptr;
    s.orig = c->orig;
    s.n_slots = c->cap > 0 ? c->n_slots : 0;
    s.n_owned = (int32_t)c->n_owned;
    return s;
}

template <int D>
inline Nodes<D> make_nodes(const double *lo, const double *hi, const int32_t *n) {
    Nodes<D> nd{};
    for (int a = 0; a < D; a++) {
        nd.n[a] = n[a];
        nd.lo[a] = lo[a];
        nd.hi[a] = n[a] == 1 ? lo[a] : hi[a];                      // a single node sits at lo
        if (n[a] > 1) nd.step[a] = (nd.hi[a] - nd.lo[a]) / (double)(n[a] - 1);
    }
    return nd;
}

// rows orthonormal, right-handed, within 1e-12
inline bool check_rot(const double *r) {
    bool ok = true;
    for (int a = 0; a < 3; a++)
        for (int b = a; b < 3; b++) {
            const double dot = (r[3 * a] * r[3 * b] + r[3 * a + 1] * r[3 * b + 1]) + r[3 * a + 2] * r[3 * b + 2];
            ok = ok && std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-12;
        }
    const double det = r[0] * (r[4] * r[8] - r[5] * r[7]) - r[1] * (r[3] * r[8] - r[5] * r[6]) + r[2] * (r[3] * r[7] - r[4] * r[6]);
    return ok && std::fabs(det - 1.0) <= 1e-12;
}

// read-back 1's h range of a selection of count particles
inline int check_h_range(sph_ctx *c, const char *who, int64_t count, double h_max, double h_min) {
    if (count > 0 && !(h_min > 0.0 && std::isfinite(h_max))) {
        c->err = std::string(who) + ": a selected particle has h <= 0 or a non-finite h";
        return SPH_ERR_STATE;
    }
    return SPH_OK;
}

// Read-back 1, after the pass's own partial kernel has been launched over nb blocks: reduces the rows of partial into
// stats on the device and brings the N statistics back into hs.  Synchronises the stream.
template <int N, int NMIN, int NMAX>
inline int stats_read_back(sph_ctx *c, const double *partial, int nb, double *stats, double (&hs)[N]) {
    stats_final<N, NMIN, NMAX><<<dim3(1), dim3(N * WAVE), 0, c->stream>>>(partial, nb, stats);
    SPH_HIP(hipGetLastError());
    SPH_HIP(hipMemcpyAsync(c->rnd_pinned, stats, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    SPH_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < N; k++) hs[k] = c->rnd_pinned[k];
    return SPH_OK;
}

}  // namespace sph
