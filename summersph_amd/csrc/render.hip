// render.hip -- the SPH density interpolant on a regular node grid: a full 3-D grid or its column sums along one axis.
//
// Replaces the grid loop and the projection of the reference's imaging script (Density_Image.py: one KD-tree ball query
// per node of a 120^3 np.linspace grid, sum of m W(r, h) with the analytic cubic spline, sum along z).  Not part of the
// step loop: nothing here reads or writes the context's grid, cell table, neighbour list, statistics or flags.
//
// Pipeline (all on ctx->stream, render-private scratch):
//   render_stats_partial, stats_final  owned gas particles inside the clip box: min/max xyz, max/min h, count  (read-back 1)
//   render_select                the selected particles within 2 h_j of the node box -> 64-bit key (cell << 32 | id)
//                                and slot, compacted with an atomic cursor                            (read-back 2)
//   rocprim radix sort           (cell, particle id): the order every node adds its terms in
//   start_table / render_records   cell table; SoA records {x, y, z, m sigma_j, 1/h_j} in sorted order
//   render_field_records         (sph_render_field) SoA records {x, y, z, w_j sigma_j, w_j sigma_j A_j, 1/h_j} in sorted order
//   render_gather<W>             one workgroup per tile of 8 x 8 node columns; lanes walk axis W in segments of KW nodes.
//                                The records of the cells that overlap a segment's brick (+ the reach) are staged into LDS
//                                in chunks, in increasing (cell, id) order, and every lane adds its KW nodes' terms in that
//                                staged order.  3-D mode stores the node values; projected mode adds them, node by node
//                                in increasing index, into the column sum and never materialises the grid.
//   field_gather<W, DEN>         (sph_render_field) the same walk and staging with a sixth plane: num += w sigma A Wn and,
//                                with DEN, den += w sigma Wn per accepted pair; the epilogue divides / scales.
// A node's value is therefore the sum of its contributing terms in the global (cell, id) order of a binning that depends
// only on the node box, n, h and the clip: independent of the context's sorted order, of the launch geometry and of the
// output mode (terms of particles beyond 2h are skipped or are exact +0.0, which changes no sum).
// The selection, the h rule, the reach, the nodes and start_table are image_common.hpp's, shared with cube.hip and transfer.hip.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>

#include "image_common.hpp"

// the 3-D values and the column sums must be bitwise the same per node: no contraction into fused multiply-adds that
// the compiler might choose differently in the three instantiations of the gather
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int RB = 256;            // reduction / select block
constexpr int RB_MAX = 1024;       // blocks of the reduction
constexpr int NSTAT = 9, NMIN = 3, NMAX = 5;       // min xyz; max xyz, max h, max(-h); count
#ifndef RENDER_TILE
#define RENDER_TILE 8              // A/B switch ("Density rendering"): 16 = workgroups of 16 x 16 columns
#endif
constexpr int TU = RENDER_TILE, TV = RENDER_TILE;   // node columns per workgroup (v fastest)
constexpr int GT = TU * TV;        // threads per gather workgroup
constexpr int KW = 8;              // nodes per lane along the walk axis per segment
constexpr int CH = 4 * GT;         // records per LDS chunk (5 planes of doubles: 10 KB for 8 x 8 columns; the field
                                   // render's 6 planes: 12 KB)
constexpr int64_t MAX_CELLS = (int64_t)1 << 26;

struct RGrid {                     // render-private cell grid
    double org[3];
    double inv_edge;
    int32_t dim[3];
};

struct Recs {
    const double *x, *y, *z, *ms, *ih;
    const int32_t *cell_start;
    const double *wa;              // the field render's w sigma A plane (unused by the density render)
};

__device__ __forceinline__ int32_t cell_1d(const RGrid &g, int a, double p) {
    const double t = floor((p - g.org[a]) * g.inv_edge);
    return (int32_t)fmin(fmax(t, 0.0), (double)(g.dim[a] - 1));     // monotone in p; NaN -> 0
}

// partial[b * NSTAT + k]: min x y z, max x y z, max h, max -h, count over block b's grid-stride share of the selection
__global__ __launch_bounds__(RB) void render_stats_partial(const double *__restrict__ x, const double *__restrict__ y,
                                                           const double *__restrict__ z, Sel s, double *__restrict__ partial) {
    double v[NSTAT] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < s.n_slots; i += (int64_t)gridDim.x * RB) {
        const double p[3] = {x[i], y[i], z[i]};
        if (!selected(s, i, p[0], p[1], p[2])) continue;
#pragma unroll
        for (int a = 0; a < 3; a++) { v[a] = fmin(v[a], p[a]); v[3 + a] = fmax(v[3 + a], p[a]); }
        const double h = sel_h(s, i);
        v[6] = fmax(v[6], h);
        v[7] = fmax(v[7], -h);
        v[8] += 1.0;
    }
    stats_block_partial<NMIN, NMAX, RB>(v, partial);
}

// the selected particles within 2 h_j (1 + 1e-6) of the node box -> key (cell << 32 | original id), slot
__global__ __launch_bounds__(RB) void render_select(const double *__restrict__ x, const double *__restrict__ y,
                                                    const double *__restrict__ z, Sel s, Nodes<3> nd, RGrid g,
                                                    uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                    uint32_t *__restrict__ cursor, int64_t cap) {
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < s.n_slots; i += (int64_t)gridDim.x * RB) {
        const double p[3] = {x[i], y[i], z[i]};
        if (!selected(s, i, p[0], p[1], p[2])) continue;
        const double reach = sel_reach(s, i);
        bool near = true;
#pragma unroll
        for (int a = 0; a < 3; a++) near = near && p[a] >= nd.lo[a] - reach && p[a] <= nd.hi[a] + reach;
        if (!near) continue;
        const uint64_t cell = ((uint64_t)cell_1d(g, 0, p[0]) * (uint64_t)g.dim[1] + (uint64_t)cell_1d(g, 1, p[1])) * (uint64_t)g.dim[2] +
                              (uint64_t)cell_1d(g, 2, p[2]);
        const uint32_t k = atomicAdd(cursor, 1u);
        if ((int64_t)k < cap) {
            keys[k] = (cell << 32) | (uint64_t)(uint32_t)s.orig[i];
            vals[k] = (uint32_t)i;
        }
    }
}

// records in sorted order: x, y, z, m sigma_j = m / (pi h_j^3), 1 / h_j   (double-precision pi: the script's kernel)
__global__ __launch_bounds__(256) void render_records(const double *__restrict__ x, const double *__restrict__ y,
                                                      const double *__restrict__ z, const double *__restrict__ m, Sel s,
                                                      const uint32_t *__restrict__ vals, int64_t n, double *__restrict__ rec,
                                                      int64_t stride) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = vals[i];
    const double h = sel_h(s, j);
    rec[i] = x[j];
    rec[stride + i] = y[j];
    rec[2 * stride + i] = z[j];
    rec[3 * stride + i] = m[j] * (1.0 / (M_PI * (h * h * h)));
    rec[4 * stride + i] = 1.0 / h;
}

// the field render's records in sorted order: x, y, z, ws = w_j sigma_j, wa = ws A_j, 1 / h_j with w_j = m_j (rho null) or
// m_j / rho_j, A_j = a[j] (a field plane in slot order) or values[orig[j]] (the caller's order).  ws of the mass weight is
// bitwise render_records' m sigma_j.
__global__ __launch_bounds__(256) void render_field_records(const double *__restrict__ x, const double *__restrict__ y,
                                                            const double *__restrict__ z, const double *__restrict__ m,
                                                            const double *__restrict__ rho, const double *__restrict__ a,
                                                            const double *__restrict__ values, Sel s,
                                                            const uint32_t *__restrict__ vals, int64_t n,
                                                            double *__restrict__ rec, int64_t stride) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = vals[i];
    const double h = sel_h(s, j);
    const double sigma = 1.0 / (M_PI * (h * h * h));
    const double ws = (rho ? m[j] / rho[j] : m[j]) * sigma;
    const double av = values ? values[s.orig[j]] : a[j];
    rec[i] = x[j];
    rec[stride + i] = y[j];
    rec[2 * stride + i] = z[j];
    rec[3 * stride + i] = ws;
    rec[4 * stride + i] = ws * av;
    rec[5 * stride + i] = 1.0 / h;
}

// m sigma W(|g - p|, h) with W/sigma = 1 - 1.5 q^2 + 0.75 q^3 (q <= 1), 0.25 (2 - q)^3 (1 < q <= 2), 0 beyond.
// The squared distance is summed in x, y, z order in every instantiation.
__device__ __forceinline__ double kernel_w(double q) {
    const double t = 2.0 - q;
    const double w1 = (1.0 - 1.5 * (q * q)) + 0.75 * (q * q * q);
    const double w2 = 0.25 * (t * t * t);
    return q <= 1.0 ? w1 : (q <= 2.0 ? w2 : 0.0);
}

struct GatherArgs {
    Nodes<3> nd;
    RGrid g;
    Recs r;
    double reach;      // 2 h_max (1 + 1e-6): the brick's box is widened by this to find its candidate cells
    double scale;      // multiplier of the column sums (node spacing or 1)
    int32_t project;   // 1: column sums along W
    int32_t tiles_v;   // tiles along V
    int32_t nseg;      // segments of KW nodes along W
    int32_t normalise; // field render: num / den (0 where den == 0), unscaled
    double *out;
    double *wout;      // field render: den (3-D) or the column den times scale; null = none
};

// W: walk axis; U < V the two others (V fastest in both outputs).  3-D mode runs W = 0: lanes then span the two fastest
// output axes and the stores of a segment are rows of TV consecutive doubles.
// FIELD: the field render (a sixth record plane wa; num += wa Wn), DEN: it also accumulates den += ws Wn.  Without FIELD
// this is the density render: acc += ms W.
template <int W, bool FIELD, bool DEN>
__device__ __forceinline__ void gather_body(const GatherArgs &A) {
    constexpr int U = W == 0 ? 1 : 0, V = W == 2 ? 1 : 2;
    __shared__ double sx[CH], sy[CH], sz[CH], sms[CH], sih[CH];
    __shared__ double swa[FIELD ? CH : 1];
    __shared__ int32_t s_start[GT], s_off[GT];
    __shared__ int32_t s_wsum[GT / WAVE];

    const Nodes<3> &nd = A.nd;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int tu = blockIdx.x / A.tiles_v, tv = blockIdx.x % A.tiles_v;
    const int iu = tu * TU + t / TV, iv = tv * TV + t % TV;
    const bool valid = iu < nd.n[U] && iv < nd.n[V];
    const double cu = node_coord(nd, U, min(iu, nd.n[U] - 1)), cv = node_coord(nd, V, min(iv, nd.n[V] - 1));
    const int u0 = tu * TU, u1 = min(nd.n[U], u0 + TU) - 1;
    const int v0 = tv * TV, v1 = min(nd.n[V], v0 + TV) - 1;
    const int d1 = A.g.dim[1], d2 = A.g.dim[2];
    double col = 0.0, cold = 0.0;

    for (int seg = blockIdx.y; seg < A.nseg; seg += gridDim.y) {
        const int w0 = seg * KW, w1 = min(nd.n[W], w0 + KW) - 1;
        double cw[KW], acc[KW], accd[DEN ? KW : 1];
#pragma unroll
        for (int k = 0; k < KW; k++) { cw[k] = node_coord(nd, W, min(w0 + k, w1)); acc[k] = 0.0; }
        if constexpr (DEN) {
#pragma unroll
            for (int k = 0; k < KW; k++) accd[k] = 0.0;
        }
        // candidate cells: the brick's box widened by the reach, in x y z
        int clo[3], chi[3];
        {
            double blo[3], bhi[3];
            blo[W] = node_coord(nd, W, w0); bhi[W] = node_coord(nd, W, w1);
            blo[U] = node_coord(nd, U, u0); bhi[U] = node_coord(nd, U, u1);
            blo[V] = node_coord(nd, V, v0); bhi[V] = node_coord(nd, V, v1);
#pragma unroll
            for (int a = 0; a < 3; a++) { clo[a] = cell_1d(A.g, a, blo[a] - A.reach); chi[a] = cell_1d(A.g, a, bhi[a] + A.reach); }
        }
        const int n1c = chi[1] - clo[1] + 1, n2c = chi[2] - clo[2] + 1;
        const int64_t n_int = (int64_t)(chi[0] - clo[0] + 1) * n1c;     // one interval of sorted records per (cx, cy)
        for (int64_t ib = 0; ib < n_int; ib += GT) {
            const int nb = (int)min<int64_t>(GT, n_int - ib);
            int start = 0, len = 0;
            if (t < nb) {
                const int64_t r = ib + t;
                const int64_t k0 = ((int64_t)(clo[0] + (int)(r / n1c)) * d1 + (clo[1] + (int)(r % n1c))) * d2 + clo[2];
                start = A.r.cell_start[k0];
                len = A.r.cell_start[k0 + n2c] - start;
            }
            int incl = len;                                    // block-wide exclusive scan of the interval lengths
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o, 64);
                if (lane >= o) incl += y;
            }
            __syncthreads();                                   // the previous batch is done with s_start / s_off
            if (lane == 63) s_wsum[wv] = incl;
            __syncthreads();
            int base = 0, total = 0;
#pragma unroll
            for (int w = 0; w < GT / WAVE; w++) { base += w < wv ? s_wsum[w] : 0; total += s_wsum[w]; }
            s_start[t] = start;
            s_off[t] = base + incl - len;
            __syncthreads();
            for (int cb = 0; cb < total; cb += CH) {
                const int cnt = min(CH, total - cb);
                for (int e = t; e < cnt; e += GT) {
                    const int pos = cb + e;
                    int lo = 0, hi = nb - 1;                   // last interval whose offset is <= pos (a non-empty one)
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (s_off[mid] <= pos) lo = mid; else hi = mid - 1;
                    }
                    const int64_t idx = (int64_t)s_start[lo] + (pos - s_off[lo]);
                    sx[e] = A.r.x[idx]; sy[e] = A.r.y[idx]; sz[e] = A.r.z[idx]; sms[e] = A.r.ms[idx]; sih[e] = A.r.ih[idx];
                    if constexpr (FIELD) swa[e] = A.r.wa[idx];
                }
                __syncthreads();
                for (int j = 0; j < cnt; j++) {                // every lane reads the same record: LDS broadcast
                    const double p[3] = {sx[j], sy[j], sz[j]};
                    const double ms = sms[j], ih = sih[j], ih2 = ih * ih;
                    const double wa = FIELD ? swa[j] : 0.0;
                    const double du = cu - p[U];
                    const double dv = cv - p[V];
#pragma unroll
                    for (int k = 0; k < KW; k++) {
                        double d[3];
                        d[U] = du; d[V] = dv; d[W] = cw[k] - p[W];
                        const double r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
                        if (r2 * ih2 <= 4.0000001) {           // beyond it q > 2: the term is +0.0, skipped
                            const double q = sqrt(r2) * ih;
                            if constexpr (FIELD) {
                                const double wn = kernel_w(q);
                                acc[k] += wa * wn;
                                if constexpr (DEN) accd[k] += ms * wn;
                            } else {
                                acc[k] += ms * kernel_w(q);
                            }
                        }
                    }
                }
                __syncthreads();
            }
        }
        if (A.project) {
#pragma unroll
            for (int k = 0; k < KW; k++)
                if (w0 + k <= w1) {
                    col += acc[k];                             // node by node, increasing index: the sequential sum
                    if constexpr (DEN) cold += accd[k];
                }
        } else if (valid) {
#pragma unroll
            for (int k = 0; k < KW; k++) {
                if (w0 + k > w1) break;
                int64_t i3[3];
                i3[W] = w0 + k; i3[U] = iu; i3[V] = iv;
                const int64_t o = (i3[0] * nd.n[1] + i3[1]) * nd.n[2] + i3[2];
                if constexpr (DEN) {
                    A.out[o] = A.normalise ? (accd[k] != 0.0 ? acc[k] / accd[k] : 0.0) : acc[k];
                    if (A.wout) A.wout[o] = accd[k];
                } else {
                    A.out[o] = acc[k];
                }
            }
        }
    }
    if (A.project && valid) {
        const int64_t o = (int64_t)iu * nd.n[V] + iv;
        if constexpr (DEN) {
            A.out[o] = A.normalise ? (cold != 0.0 ? col / cold : 0.0) : col * A.scale;
            if (A.wout) A.wout[o] = cold * A.scale;
        } else {
            A.out[o] = col * A.scale;
        }
    }
}

template <int W>
__global__ __launch_bounds__(GT) void render_gather(GatherArgs A) { gather_body<W, false, false>(A); }

// the field render's gather (sph_render_field): its name must not contain the density gather's
template <int W, bool DEN>
__global__ __launch_bounds__(GT) void field_gather(GatherArgs A) { gather_body<W, true, DEN>(A); }

template <int W>
hipError_t launch_gather(const GatherArgs &a, int tiles, int ysegs, hipStream_t st) {
    render_gather<W><<<dim3((unsigned)tiles, (unsigned)ysegs), dim3(GT), 0, st>>>(a);
    return hipGetLastError();
}

template <int W>
hipError_t launch_field_gather(const GatherArgs &a, bool den, int tiles, int ysegs, hipStream_t st) {
    if (den) field_gather<W, true><<<dim3((unsigned)tiles, (unsigned)ysegs), dim3(GT), 0, st>>>(a);
    else field_gather<W, false><<<dim3((unsigned)tiles, (unsigned)ysegs), dim3(GT), 0, st>>>(a);
    return hipGetLastError();
}

// what sph_render_field adds to the density render's pipeline
struct FieldSpec {
    const double *a;           // the field's plane (slot order), or null
    const double *values;      // the caller's values (original order; host memory when host_values), or null
    bool host_values;
    const double *rho;         // VOLUME weight: the rho plane; null = MASS
    bool normalise;
    double *wout;              // weight output (host or device, as the image), or null
    bool stale;                // the field or rho would be refused by sph_download_field
};

// the density render (fs null) and the field render: shared selection, binning, sort and cells; records and gather differ
int render_impl(sph_ctx *c, sph_render_desc *d, const FieldSpec *fs, double *out, int64_t out_len, bool host_out) {
    const char *who = fs ? "sph_render_field" : "sph_render_density";
    if (!d || !out) return arg_error(c, who, "null descriptor or output");
    if (d->reserved != 0) return arg_error(c, who, "reserved must be 0");
    if (d->flags & ~(SPH_RENDER_AUTO_BOUNDS | SPH_RENDER_SPACING)) return arg_error(c, who, "unknown flags");
    const bool autob = (d->flags & SPH_RENDER_AUTO_BOUNDS) != 0, spacing = (d->flags & SPH_RENDER_SPACING) != 0;
    int64_t total = 1;
    for (int a = 0; a < 3; a++) {
        if (d->n[a] < 1) return arg_error(c, who, "n must be >= 1 on every axis");
        total *= d->n[a];
        if (total > ((int64_t)1 << 40)) return arg_error(c, who, "too many nodes");
    }
    if (d->axis < -1 || d->axis > 2) return arg_error(c, who, "axis must be -1, 0, 1 or 2");
    if (spacing && (d->axis < 0 || d->n[d->axis] == 1)) return arg_error(c, who, "SPH_RENDER_SPACING needs a projection axis with n > 1");
    if (!(d->h >= 0.0) || !std::isfinite(d->h)) return arg_error(c, who, "h must be finite and >= 0");
    const int64_t want = d->axis < 0 ? total : total / d->n[d->axis];
    if (out_len != want) return arg_error(c, who, "out_len does not match the node counts");
    if (!autob)
        for (int a = 0; a < 3; a++)
            if (!(d->lo[a] <= d->hi[a]) || !std::isfinite(d->lo[a]) || !std::isfinite(d->hi[a])) return arg_error(c, who, "lo > hi");
    for (int a = 0; a < 3; a++)
        if (std::isnan(d->clip_lo[a]) || std::isnan(d->clip_hi[a])) return arg_error(c, who, "NaN clip box");
    if (fs && fs->stale) {
        c->err = "sph_render_field: the field or rho is stale (sph_download_field would refuse it)";
        return SPH_ERR_STATE;
    }

    hipStream_t st = c->stream;
    const Sel s = make_sel(c, d->clip_lo, d->clip_hi, d->h);

    if (!c->rnd_small) SPH_TRY(ctx_alloc(c, &c->rnd_small, (size_t)RB_MAX * NSTAT + 16, "render statistics"));
    SPH_TRY(analysis_pinned(c));
    double *stats = c->rnd_small + (size_t)RB_MAX * NSTAT;
    uint32_t *cursor = reinterpret_cast<uint32_t *>(stats + NSTAT + 1);

    // ---- read-back 1: the selection's box, h range and size ----------------------------------------------------------
    double hs[NSTAT] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
    if (s.n_slots > 0) {
        const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((s.n_slots + RB - 1) / RB, RB_MAX));
        render_stats_partial<<<dim3(nb), dim3(RB), 0, st>>>(c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], s, c->rnd_small);
        SPH_TRY((stats_read_back<NSTAT, NMIN, NMAX>(c, c->rnd_small, nb, stats, hs)));
    }
    const int64_t count = (int64_t)hs[8];
    if (count == 0 && autob) return arg_error(c, who, "SPH_RENDER_AUTO_BOUNDS over an empty selection");
    const double h_max = hs[6], h_min = -hs[7];
    SPH_TRY(check_h_range(c, who, count, h_max, h_min));
    const double *lo = autob ? hs : d->lo, *hi = autob ? hs + 3 : d->hi;
    const Nodes<3> nd = make_nodes<3>(lo, hi, d->n);

    // ---- render grid: edge max(2 h_max, what keeps the table within MAX_CELLS) over the node box + the reach -----------
    RGrid g{};
    double reach = 0.0;
    int64_t ncells = 1;
    if (count > 0) {
        reach = reach_of(h_max);
        double ext[3], edge = 2.0 * h_max;
        for (int a = 0; a < 3; a++) { g.org[a] = nd.lo[a] - reach; ext[a] = (nd.hi[a] + reach) - g.org[a]; }
        for (;;) {
            double prod = 1.0;
            for (int a = 0; a < 3; a++) prod *= std::max(1.0, std::ceil(ext[a] / edge));
            if (prod <= (double)MAX_CELLS) break;
            edge *= 1.2599210498948732;                   // 2^(1/3): halves the table
        }
        ncells = 1;
        for (int a = 0; a < 3; a++) { g.dim[a] = (int32_t)std::max(1.0, std::ceil(ext[a] / edge)); ncells *= g.dim[a]; }
        g.inv_edge = 1.0 / edge;
    }

    // ---- scratch ----------------------------------------------------------------------------------------------------
    const int64_t cap = std::max<int64_t>(count, 1);
    size_t sort_bytes = 0;
    SPH_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)cap, 0u, 64u, st));
    const int nplanes = fs ? 6 : 5;
    const bool host_w = fs && fs->wout && host_out, host_v = fs && fs->values && fs->host_values;
    uint64_t *keys, *keys_alt;
    uint32_t *vals, *vals_alt;
    char *sort_tmp;
    int32_t *cell_start;
    double *rec, *h_out, *h_wout, *values_copy;
    auto layout = [&](Carve cv) {
        keys = cv.take<uint64_t>(cap);
        keys_alt = cv.take<uint64_t>(cap);
        vals = cv.take<uint32_t>(cap);
        vals_alt = cv.take<uint32_t>(cap);
        sort_tmp = cv.take<char>(sort_bytes);
        cell_start = cv.take<int32_t>(ncells + 2);
        rec = cv.take<double>((size_t)nplanes * (size_t)cap);
        h_out = cv.take<double>(host_out ? out_len : 0);              // the host form's device copies
        h_wout = cv.take<double>(host_w ? out_len : 0);
        values_copy = cv.take<double>(host_v ? std::max<int64_t>(c->n, 0) : 0);     // the host form's values, on the device
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    double *d_out = host_out ? h_out : out;
    double *d_wout = host_w ? h_wout : (fs ? fs->wout : nullptr);
    const double *d_values = host_v ? values_copy : (fs ? fs->values : nullptr);

    // ---- read-back 2: the particles that can reach a node -----------------------------------------------------------
    int64_t nsel = 0;
    if (count > 0) {
        SPH_HIP(hipMemsetAsync(cursor, 0, sizeof(uint32_t), st));
        const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((s.n_slots + RB - 1) / RB, 4 * RB_MAX));
        render_select<<<dim3(nb), dim3(RB), 0, st>>>(c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], s, nd, g, keys, vals, cursor, cap);
        SPH_HIP(hipGetLastError());
        SPH_HIP(hipMemcpyAsync(c->rnd_pinned + 16, cursor, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));
        nsel = std::min<int64_t>(*reinterpret_cast<const uint32_t *>(c->rnd_pinned + 16), cap);
    }

    if (nsel == 0) {
        SPH_HIP(hipMemsetAsync(d_out, 0, (size_t)out_len * sizeof(double), st));
        if (d_wout) SPH_HIP(hipMemsetAsync(d_wout, 0, (size_t)out_len * sizeof(double), st));
    } else {
        unsigned cbits = 1;
        while (cbits < 32 && ((int64_t)1 << cbits) < ncells) cbits++;
        size_t tmp = sort_bytes;
        SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, keys, keys_alt, vals, vals_alt, (size_t)nsel, 0u, 32u + cbits, st));
        start_table<<<dim3((unsigned)((ncells + 1 + 255) / 256)), dim3(256), 0, st>>>(keys_alt, nsel, ncells, cell_start);
        if (!fs) {
            render_records<<<dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, st>>>(c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z],
                                                                                       c->f[SPH_F_M], s, vals_alt, nsel, rec, cap);
        } else {
            if (host_v) SPH_HIP(hipMemcpyAsync(values_copy, fs->values, (size_t)c->n * sizeof(double), hipMemcpyHostToDevice, st));
            render_field_records<<<dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, st>>>(
                c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], c->f[SPH_F_M], fs->rho, fs->a, d_values, s, vals_alt, nsel, rec, cap);
        }
        SPH_HIP(hipGetLastError());
        GatherArgs a{};
        a.nd = nd; a.g = g; a.reach = reach;
        if (!fs) a.r = Recs{rec, rec + cap, rec + 2 * cap, rec + 3 * cap, rec + 4 * cap, cell_start, nullptr};
        else a.r = Recs{rec, rec + cap, rec + 2 * cap, rec + 3 * cap, rec + 5 * cap, cell_start, rec + 4 * cap};
        a.project = d->axis >= 0;
        const int W = d->axis >= 0 ? d->axis : 0, U = W == 0 ? 1 : 0, V = W == 2 ? 1 : 2;
        a.scale = spacing ? nd.step[W] : 1.0;
        a.tiles_v = (nd.n[V] + TV - 1) / TV;
        a.nseg = (nd.n[W] + KW - 1) / KW;
        a.out = d_out;
        a.wout = d_wout;
        a.normalise = fs && fs->normalise;
        const int64_t tiles = (int64_t)((nd.n[U] + TU - 1) / TU) * a.tiles_v;
        if (tiles > 0x7fffffff) return arg_error(c, "sph_render_density", "too many node columns");
        const int ysegs = a.project ? 1 : std::min(a.nseg, 65535);
        if (!fs) {
            SPH_HIP(W == 0 ? launch_gather<0>(a, (int)tiles, ysegs, st)
                           : (W == 1 ? launch_gather<1>(a, (int)tiles, ysegs, st) : launch_gather<2>(a, (int)tiles, ysegs, st)));
        } else {
            const bool den = fs->normalise || fs->wout;
            SPH_HIP(W == 0 ? launch_field_gather<0>(a, den, (int)tiles, ysegs, st)
                           : (W == 1 ? launch_field_gather<1>(a, den, (int)tiles, ysegs, st)
                                     : launch_field_gather<2>(a, den, (int)tiles, ysegs, st)));
        }
    }
    if (host_out) {
        SPH_HIP(hipMemcpyAsync(out, d_out, (size_t)out_len * sizeof(double), hipMemcpyDeviceToHost, st));
        if (host_w) SPH_HIP(hipMemcpyAsync(fs->wout, d_wout, (size_t)out_len * sizeof(double), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));
    }
    if (autob)
        for (int a = 0; a < 3; a++) { d->lo[a] = hs[a]; d->hi[a] = hs[3 + a]; }
    return SPH_OK;
}

}  // namespace

// the analysis calls' scratch: grows, never shrinks; freed with the context.  A grown buffer replaces the old one only
// after the stream has drained (a previous _dev call may still read it).
int analysis_scratch(sph_ctx *c, size_t bytes, char **out) {
    if (bytes > c->rnd_bytes) {
        SPH_HIP(hipStreamSynchronize(c->stream));
        ctx_free_ptr(c, c->rnd_buf); c->rnd_buf = nullptr; c->rnd_bytes = 0;
        SPH_TRY(ctx_alloc_bytes(c, &c->rnd_buf, bytes, "render scratch"));
        c->rnd_bytes = bytes;
    }
    *out = static_cast<char *>(c->rnd_buf);
    return SPH_OK;
}

int analysis_pinned(sph_ctx *c) {
    if (!c->rnd_pinned) SPH_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->rnd_pinned), 32 * sizeof(double), hipHostMallocDefault));
    return SPH_OK;
}

void render_free(sph_ctx *c) {
    ctx_free_ptr(c, c->rnd_buf); c->rnd_buf = nullptr; c->rnd_bytes = 0;
    ctx_free(c, c->rnd_small);
    if (c->rnd_pinned) (void)hipHostFree(c->rnd_pinned);
    c->rnd_pinned = nullptr;
}

int render_density(sph_ctx *c, sph_render_desc *d, double *out, int64_t out_len, bool host_out) {
    return render_impl(c, d, nullptr, out, out_len, host_out);
}

int render_field(sph_ctx *c, sph_render_field_desc *d, const double *values, double *out, double *wout, int64_t out_len,
                 bool host) {
    const char *who = "sph_render_field";
    if (!d) return arg_error(c, who, "null descriptor");
    if (d->reserved != 0) return arg_error(c, who, "reserved must be 0");
    if (d->field < SPH_RENDER_FIELD_VALUES || d->field >= SPH_F_COUNT) return arg_error(c, who, "field id out of range");
    if ((d->field == SPH_RENDER_FIELD_VALUES) != (values != nullptr))
        return arg_error(c, who, "values must be given with SPH_RENDER_FIELD_VALUES and only then");
    if (d->weight != SPH_RENDER_WEIGHT_MASS && d->weight != SPH_RENDER_WEIGHT_VOLUME) return arg_error(c, who, "unknown weight");
    if (d->normalise != 0 && d->normalise != 1) return arg_error(c, who, "normalise must be 0 or 1");
    const bool volume = d->weight == SPH_RENDER_WEIGHT_VOLUME;
    FieldSpec fs{};
    fs.a = d->field >= 0 ? c->f[d->field] : nullptr;
    fs.values = values;
    fs.host_values = host;
    fs.rho = volume ? c->f[SPH_F_RHO] : nullptr;
    fs.normalise = d->normalise != 0;
    fs.wout = wout;
    fs.stale = (d->field >= 0 && !field_ready(*c, c->variable, d->field)) || (volume && !field_ready(*c, c->variable, SPH_F_RHO));
    return render_impl(c, &d->base, &fs, out, out_len, host);
}

}  // namespace sph
