// cube.hip -- sph_cube: the optically thin position-position-velocity cube of the owned gas seen along any direction.
//
// voxel[k][iu][iv] = sum_j Y_j(|node - P_j,uv|) (cdf_j(e_{k+1}) - cdf_j(e_k)): the cubic spline integrated along the line
// of sight analytically (F, below) as the spatial footprint, a Gaussian of width sigma_j about the particle's line-of-sight
// velocity as the line profile (include/summersph.h, "spectral cubes", has the definition).  Not part of the step loop:
// nothing here reads or writes the context's grid, cell table, neighbour list, statistics or flags.
//
// Pipeline (all on ctx->stream, the analysis calls' scratch), the density render's front end in the image plane:
//   cube_stats_partial, stats_final  owned gas particles inside the clip box: max h, min h, count          (read-back 1)
//   cube_select                P_j = rot (r_j - centre); the selected particles within 2 h_j of the node box -> 64-bit key
//                              (image-plane cell << 32 | id) and slot, compacted with an atomic cursor     (read-back 2)
//   rocprim radix sort         (cell, particle id): the order every voxel adds its terms in
//   start_table / cube_records cell table; SoA records {P_u, P_v, V, m A / (pi h^2), 1 / h, sigma} and the particle's
//                              channel range [klo, khi] (outside it every weight is an exact +0.0), in sorted order
//   cube_gather                one wavefront per tile of 8 x 8 image nodes and per chunk of CC channels.  Every lane keeps
//                              its node's CC-channel spectrum in LDS (slot [channel][lane]: lanes own disjoint slots, no
//                              atomics).  The records of the cells that overlap the tile (+ the reach) are staged into LDS
//                              in (cell, id) order; records whose channel range misses the chunk, or whose footprint
//                              misses all 64 nodes, are skipped.  For the others the 64 lanes compute the cdf at one
//                              channel edge each (the weights depend on the particle only), the lanes inside the footprint
//                              evaluate F once and add Y w_k into their own slots, w_k read from the lane that holds it.
// A voxel's value is therefore the sum of its terms in the (cell, id) order of a binning that depends only on the
// descriptor and the selected particles' h range: bitwise reproducible and independent of the context's sorted order.
// The selection, the h rule, the reach, the nodes, the frame and start_table are image_common.hpp's, shared with render.hip
// and transfer.hip.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>

#include "image_common.hpp"
#include "spline_column.hpp"

// the definition fixes the order of the frame's sums; no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int RB = 256;            // reduction / select block
constexpr int RB_MAX = 1024;       // blocks of the reduction
constexpr int NSTAT = 3, NMIN = 0, NMAX = 2;       // max h, max(-h); count
constexpr int TU = 8, TV = 8;      // image nodes per workgroup (v fastest)
constexpr int GT = TU * TV;        // threads per gather workgroup: one wavefront
static_assert(GT == WAVE, "cube_gather passes the channel weights between the lanes of one wavefront");
#ifndef CUBE_CHUNK
#define CUBE_CHUNK 32              // A/B switch ("Spectral cubes"): channels of a node's spectrum kept in LDS
#endif
constexpr int CC = CUBE_CHUNK;     // 32 channels x 64 lanes x 8 B = 16 KB
static_assert(CC >= 1 && CC < WAVE, "one lane per channel edge of a chunk");
constexpr int CH = 2 * GT;         // records per LDS stage (6 planes of doubles + 2 of ints: 7 KB)
constexpr int64_t MAX_CELLS = (int64_t)1 << 22;
constexpr double XCUT = 8.5;       // the line profile's truncation, in sigma

struct VFrame : Frame {            // the frame and its velocity zero (a kernel argument: sph_transfer's frame has none)
    double v_ref[3];
};

struct PGrid {                     // image-plane cell grid
    double org[2];
    double inv_edge;
    int32_t dim[2];
};

struct Chan {
    double v0, dv;
    double sigma_scale, sigma_floor;
    int32_t n;
};

__device__ __forceinline__ int32_t cell_1d(const PGrid &g, int a, double p) {
    const double t = floor((p - g.org[a]) * g.inv_edge);
    return (int32_t)fmin(fmax(t, 0.0), (double)(g.dim[a] - 1));     // monotone in p; NaN -> 0
}

// partial[b * NSTAT + k]: max h, max -h, count over block b's grid-stride share of the selection
__global__ __launch_bounds__(RB) void cube_stats_partial(const double *__restrict__ x, const double *__restrict__ y,
                                                         const double *__restrict__ z, Sel s, double *__restrict__ partial) {
    double v[NSTAT] = {-INFINITY, -INFINITY, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < s.n_slots; i += (int64_t)gridDim.x * RB) {
        if (!selected(s, i, x[i], y[i], z[i])) continue;
        const double h = sel_h(s, i);
        v[0] = fmax(v[0], h);
        v[1] = fmax(v[1], -h);
        v[2] += 1.0;
    }
    stats_block_partial<NMIN, NMAX, RB>(v, partial);
}

// the selected particles within 2 h_j (1 + 1e-6) of the node box in the image plane -> key (cell << 32 | original id), slot
__global__ __launch_bounds__(RB) void cube_select(const double *__restrict__ x, const double *__restrict__ y,
                                                  const double *__restrict__ z, Sel s, VFrame fr, Nodes<2> nd, PGrid g,
                                                  uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                  uint32_t *__restrict__ cursor, int64_t cap) {
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < s.n_slots; i += (int64_t)gridDim.x * RB) {
        const double px = x[i], py = y[i], pz = z[i];
        if (!selected(s, i, px, py, pz)) continue;
        const double dx = px - fr.centre[0], dy = py - fr.centre[1], dz = pz - fr.centre[2];
        const double P[2] = {row_dot(fr.rot, 0, dx, dy, dz), row_dot(fr.rot, 1, dx, dy, dz)};
        const double reach = sel_reach(s, i);
        bool near = true;
#pragma unroll
        for (int a = 0; a < 2; a++) near = near && P[a] >= nd.lo[a] - reach && P[a] <= nd.hi[a] + reach;
        if (!near) continue;
        const uint64_t cell = (uint64_t)cell_1d(g, 0, P[0]) * (uint64_t)g.dim[1] + (uint64_t)cell_1d(g, 1, P[1]);
        const uint32_t k = atomicAdd(cursor, 1u);
        if ((int64_t)k < cap) {
            keys[k] = (cell << 32) | (uint64_t)(uint32_t)s.orig[i];
            vals[k] = (uint32_t)i;
        }
    }
}

struct Fields {
    const double *x, *y, *z, *vx, *vy, *vz, *m, *cs;
    const double *values;          // the caller's A in the original order, or null (A = 1)
};

// channel edge k: e_k = (k - 0.5) dv + v0
__device__ __forceinline__ double chan_edge(const Chan &ch, int k) { return ((double)k - 0.5) * ch.dv + ch.v0; }

// records in sorted order: P_u, P_v, V, y0 = m A / (pi h^2), 1 / h, sigma; klo .. khi: the channels whose weight can be
// non-zero (one channel of margin on either side: the skipped ones have both edges beyond the truncation, or on one side of
// V where sigma == 0, an exact +0.0)
__global__ __launch_bounds__(256) void cube_records(Fields f, Sel s, VFrame fr, Chan ch, const uint32_t *__restrict__ vals,
                                                    int64_t n, double *__restrict__ rec, int32_t *__restrict__ krange,
                                                    int64_t stride) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = vals[i];
    const double h = sel_h(s, j);
    const double dx = f.x[j] - fr.centre[0], dy = f.y[j] - fr.centre[1], dz = f.z[j] - fr.centre[2];
    const double V = row_dot(fr.rot, 2, f.vx[j] - fr.v_ref[0], f.vy[j] - fr.v_ref[1], f.vz[j] - fr.v_ref[2]);
    double sg = ch.sigma_floor;
    if (ch.sigma_scale != 0.0) {
        const double sc = ch.sigma_scale * f.cs[j];
        sg = sqrt(sc * sc + ch.sigma_floor * ch.sigma_floor);
    }
    const double a = f.values ? f.values[s.orig[j]] : 1.0;
    rec[i] = row_dot(fr.rot, 0, dx, dy, dz);
    rec[stride + i] = row_dot(fr.rot, 1, dx, dy, dz);
    rec[2 * stride + i] = V;
    rec[3 * stride + i] = (f.m[j] * a) / (M_PI * (h * h));
    rec[4 * stride + i] = 1.0 / h;
    rec[5 * stride + i] = sg;
    // e_k <= V - XCUT sg  <=>  k <= (V - XCUT sg - v0) / dv + 0.5
    const double nmax = (double)(ch.n - 1);
    const double a_lo = floor((V - XCUT * sg - ch.v0) / ch.dv + 0.5) - 2.0;
    const double a_hi = ceil((V + XCUT * sg - ch.v0) / ch.dv + 0.5) + 1.0;
    // NaN (a non-finite velocity or sigma) keeps the whole range: the NaN then reaches the voxels as it would in the sum
    krange[i] = a_lo > 0.0 ? (int32_t)fmin(a_lo, nmax + 1.0) : 0;
    krange[stride + i] = a_hi < nmax ? (int32_t)fmax(a_hi, -1.0) : ch.n - 1;
}

// cdf of the truncated Gaussian at edge e: erf(x / sqrt 2) / 2 for |x| < XCUT, exactly +-1/2 beyond; sigma == 0: the step
__device__ __forceinline__ double line_cdf(double e, double V, double sg) {
    if (sg > 0.0) {
        const double xx = (e - V) / sg;
        if (xx >= XCUT) return 0.5;
        if (xx <= -XCUT) return -0.5;
        return 0.5 * erf(xx * M_SQRT1_2);
    }
    return e > V ? 0.5 : -0.5;     // e_k <= V < e_{k+1}
}

#ifndef CUBE_WEIGHTS_PER_LANE
// v of lane l, l the same in every lane
__device__ __forceinline__ double lane_value(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
#endif

struct GatherArgs {
    Nodes<2> nd;
    PGrid g;
    Chan ch;
    const double *pu, *pv, *vl, *y0, *ih, *sg;
    const int32_t *klo, *khi;
    const int32_t *cell_start;
    double reach;      // 2 h_max (1 + 1e-6): the tile's box is widened by this to find its candidate cells
    int32_t tiles_v;   // tiles along v
    int32_t per_velocity;   // SPH_CUBE_PER_VELOCITY: the voxels are divided by dv
    double *out;
};

// blockIdx.x: tile of TU x TV nodes; blockIdx.y: chunk of CC channels
__global__ __launch_bounds__(GT) void cube_gather(GatherArgs A) {
    __shared__ double spec[CC * GT];
    __shared__ double su[CH], sv[CH], svl[CH], sy0[CH], sih[CH], ssg[CH];
    __shared__ int32_t sklo[CH], skhi[CH];
    __shared__ int32_t s_start[GT], s_off[GT];

    const Nodes<2> &nd = A.nd;
    const int t = threadIdx.x;
    const int tu = blockIdx.x / A.tiles_v, tv = blockIdx.x % A.tiles_v;
    const int iu = tu * TU + t / TV, iv = tv * TV + t % TV;
    const bool valid = iu < nd.n[0] && iv < nd.n[1];
    const double cu = node_coord(nd, 0, min(iu, nd.n[0] - 1)), cv = node_coord(nd, 1, min(iv, nd.n[1] - 1));
    const int u0 = tu * TU, u1 = min(nd.n[0], u0 + TU) - 1;
    const int v0 = tv * TV, v1 = min(nd.n[1], v0 + TV) - 1;
    const int c0 = blockIdx.y * CC, c1 = min(A.ch.n, c0 + CC) - 1;      // this chunk's channels
    const int d1 = A.g.dim[1];

#pragma unroll
    for (int k = 0; k < CC; k++) spec[k * GT + t] = 0.0;

    // candidate cells: the tile's box widened by the reach; one interval of sorted records per cell row
    const int clo0 = cell_1d(A.g, 0, node_coord(nd, 0, u0) - A.reach), chi0 = cell_1d(A.g, 0, node_coord(nd, 0, u1) + A.reach);
    const int clo1 = cell_1d(A.g, 1, node_coord(nd, 1, v0) - A.reach), chi1 = cell_1d(A.g, 1, node_coord(nd, 1, v1) + A.reach);
    const int n_int = chi0 - clo0 + 1;
    for (int ib = 0; ib < n_int; ib += GT) {
        const int nb = min(GT, n_int - ib);
        int start = 0, len = 0;
        if (t < nb) {
            const int64_t k0 = (int64_t)(clo0 + ib + t) * d1 + clo1;
            start = A.cell_start[k0];
            len = A.cell_start[k0 + (chi1 - clo1 + 1)] - start;
        }
        int incl = len;                                        // exclusive scan of the interval lengths over the wavefront
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64);
            if (t >= o) incl += y;
        }
        const int total = __shfl(incl, 63, 64);
        __syncthreads();                                       // the previous batch is done with s_start / s_off
        s_start[t] = start;
        s_off[t] = incl - len;
        __syncthreads();
        for (int cb = 0; cb < total; cb += CH) {
            const int cnt = min(CH, total - cb);
            for (int e = t; e < cnt; e += GT) {
                const int pos = cb + e;
                int lo = 0, hi = nb - 1;                       // last interval whose offset is <= pos (a non-empty one)
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_off[mid] <= pos) lo = mid; else hi = mid - 1;
                }
                const int64_t idx = (int64_t)s_start[lo] + (pos - s_off[lo]);
                su[e] = A.pu[idx]; sv[e] = A.pv[idx]; svl[e] = A.vl[idx]; sy0[e] = A.y0[idx]; sih[e] = A.ih[idx]; ssg[e] = A.sg[idx];
                sklo[e] = A.klo[idx]; skhi[e] = A.khi[idx];
            }
            __syncthreads();
            for (int j = 0; j < cnt; j++) {                    // every lane reads the same record: LDS broadcast
                // the part of the record's channel range inside this chunk
                const int ka = __builtin_amdgcn_readfirstlane(max(sklo[j], c0));
                const int kb = __builtin_amdgcn_readfirstlane(min(skhi[j], c1));
                if (ka > kb) continue;
                const double du = cu - su[j], dv = cv - sv[j];
                const double ih = sih[j];
                const double b2 = du * du + dv * dv;
                const bool hit = b2 * (ih * ih) <= 4.0000001;  // beyond it p > 2: the term is +0.0, skipped
                if (__ballot(hit) == 0) continue;
                const double V = svl[j], sg = ssg[j];
#ifndef CUBE_WEIGHTS_PER_LANE
                // lane l: the cdf at edge ka + l, then the weight of channel ka + l (at most CC + 1 <= 64 edges)
                const double cdf = line_cdf(chan_edge(A.ch, ka + t), V, sg);
                const double w = __shfl_down(cdf, 1, 64) - cdf;
                double y = 0.0;
                if (hit) y = sy0[j] * spline_column(sqrt(b2) * ih);
                for (int k = ka; k <= kb; k++) {
                    const double wk = lane_value(w, k - ka);   // read with every lane active: a lane outside the footprint
                    if (hit) spec[(k - c0) * GT + t] += y * wk;    // may hold the weight
                }
#else
                // A/B ("Spectral cubes"): every lane inside the footprint computes the weights itself
                if (hit) {
                    const double y = sy0[j] * spline_column(sqrt(b2) * ih);
                    double prev = line_cdf(chan_edge(A.ch, ka), V, sg);
                    for (int k = ka; k <= kb; k++) {
                        const double next = line_cdf(chan_edge(A.ch, k + 1), V, sg);
                        spec[(k - c0) * GT + t] += y * (next - prev);
                        prev = next;
                    }
                }
#endif
            }
            __syncthreads();
        }
    }
    if (valid) {
        const int64_t plane = (int64_t)nd.n[0] * nd.n[1];
        const int64_t o = (int64_t)iu * nd.n[1] + iv;
        for (int k = c0; k <= c1; k++) {
            const double v = spec[(k - c0) * GT + t];
            A.out[(int64_t)k * plane + o] = A.per_velocity ? v / A.ch.dv : v;
        }
    }
}

}  // namespace

int cube_run(sph_ctx *c, const sph_cube_desc *d, const double *values, double *out, int64_t out_len, bool host) {
    const char *who = "sph_cube";
    if (!d || !out) return arg_error(c, who, "null descriptor or output");
    if (d->reserved != 0) return arg_error(c, who, "reserved must be 0");
    if (d->flags & ~SPH_CUBE_PER_VELOCITY) return arg_error(c, who, "unknown flags");
    if (d->n_u < 1 || d->n_v < 1) return arg_error(c, who, "n_u and n_v must be >= 1");
    if (d->n_chan < 1) return arg_error(c, who, "n_chan must be >= 1");
    const int64_t pixels = (int64_t)d->n_u * d->n_v;
    if (pixels > ((int64_t)1 << 40) / d->n_chan) return arg_error(c, who, "too many voxels");
    if (out_len != pixels * d->n_chan) return arg_error(c, who, "out_len does not match n_chan n_u n_v");
    if (!(d->h >= 0.0) || !std::isfinite(d->h)) return arg_error(c, who, "h must be finite and >= 0");
    for (int a = 0; a < 2; a++)
        if (!(d->lo[a] <= d->hi[a]) || !std::isfinite(d->lo[a]) || !std::isfinite(d->hi[a])) return arg_error(c, who, "lo > hi");
    for (int a = 0; a < 3; a++) {
        if (std::isnan(d->clip_lo[a]) || std::isnan(d->clip_hi[a])) return arg_error(c, who, "NaN clip box");
        if (!std::isfinite(d->centre[a]) || !std::isfinite(d->v_ref[a])) return arg_error(c, who, "centre and v_ref must be finite");
    }
    if (!(d->dv > 0.0) || !std::isfinite(d->dv) || !std::isfinite(d->v0)) return arg_error(c, who, "dv must be finite and > 0, v0 finite");
    if (!(d->sigma_scale >= 0.0) || !(d->sigma_floor >= 0.0) || !std::isfinite(d->sigma_scale) || !std::isfinite(d->sigma_floor))
        return arg_error(c, who, "sigma_scale and sigma_floor must be finite and >= 0");
    if (!check_rot(d->rot)) return arg_error(c, who, "rot must be orthonormal and right-handed within 1e-12");
    if (d->sigma_scale != 0.0 && !field_ready(*c, c->variable, SPH_F_C)) {
        c->err = "sph_cube: c is stale (sph_download_field would refuse it) and sigma_scale > 0";
        return SPH_ERR_STATE;
    }

    hipStream_t st = c->stream;
    const Sel s = make_sel(c, d->clip_lo, d->clip_hi, d->h);
    VFrame fr{};
    for (int a = 0; a < 3; a++) { fr.centre[a] = d->centre[a]; fr.v_ref[a] = d->v_ref[a]; }
    for (int a = 0; a < 9; a++) fr.rot[a] = d->rot[a];
    Chan ch{d->v0, d->dv, d->sigma_scale, d->sigma_floor, d->n_chan};

    SPH_TRY(analysis_pinned(c));
    // ---- scratch, first part: the statistics and the cursor (the rest is sized by them) -------------------------------
    double *partial, *stats;
    uint32_t *cursor;
    auto head = [&](Carve &cv) {
        partial = cv.take<double>((size_t)RB_MAX * NSTAT);
        stats = cv.take<double>(NSTAT + 1);
        cursor = cv.take<uint32_t>(1);
    };
    char *buf = nullptr;
    {
        Carve cv{};
        head(cv);
        SPH_TRY(analysis_scratch(c, cv.bytes, &buf));
        cv = Carve{buf};
        head(cv);
    }

    // ---- read-back 1: the selection's h range and size ---------------------------------------------------------------
    double hs[NSTAT] = {-INFINITY, -INFINITY, 0.0};
    if (s.n_slots > 0) {
        const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((s.n_slots + RB - 1) / RB, RB_MAX));
        cube_stats_partial<<<dim3(nb), dim3(RB), 0, st>>>(c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], s, partial);
        SPH_TRY((stats_read_back<NSTAT, NMIN, NMAX>(c, partial, nb, stats, hs)));
    }
    const int64_t count = (int64_t)hs[2];
    const double h_max = hs[0], h_min = -hs[1];
    SPH_TRY(check_h_range(c, who, count, h_max, h_min));
    const int32_t n_uv[2] = {d->n_u, d->n_v};
    const Nodes<2> nd = make_nodes<2>(d->lo, d->hi, n_uv);

    // ---- image-plane grid over the node box + the reach: edge 2 h_max, halved while a cell still spans a tile of nodes and
    //      an eighth of the reach (finer cells only trim the candidates of a tile) and the table stays within MAX_CELLS ------
    PGrid g{};
    double reach = 0.0;
    int64_t ncells = 1;
    if (count > 0) {
        reach = reach_of(h_max);
        double ext[2], edge = 2.0 * h_max;
        for (int a = 0; a < 2; a++) { g.org[a] = nd.lo[a] - reach; ext[a] = (nd.hi[a] + reach) - g.org[a]; }
        auto cells = [&](double e) { return std::max(1.0, std::ceil(ext[0] / e)) * std::max(1.0, std::ceil(ext[1] / e)); };
        while (cells(edge) > (double)MAX_CELLS) edge *= 1.4142135623730951;      // 2^(1/2): halves the table
        const double tile = std::max((double)TU * nd.step[0], (double)TV * nd.step[1]);
        while (tile > 0.0 && 0.5 * edge >= tile && 0.5 * edge >= 0.125 * reach && cells(0.5 * edge) <= (double)MAX_CELLS) edge *= 0.5;
        for (int a = 0; a < 2; a++) g.dim[a] = (int32_t)std::max(1.0, std::ceil(ext[a] / edge));
        ncells = (int64_t)g.dim[0] * g.dim[1];
        g.inv_edge = 1.0 / edge;
    }

    // ---- scratch, the rest ----------------------------------------------------------------------------------------------
    const int64_t cap = std::max<int64_t>(count, 1);
    size_t sort_bytes = 0;
    SPH_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)cap, 0u, 64u, st));
    const bool host_v = values && host;
    uint64_t *keys, *keys_alt;
    uint32_t *vals, *vals_alt;
    char *sort_tmp;
    int32_t *cell_start, *krange;
    double *rec, *h_out, *values_copy;
    auto layout = [&](Carve cv) {
        head(cv);
        keys = cv.take<uint64_t>(cap);
        keys_alt = cv.take<uint64_t>(cap);
        vals = cv.take<uint32_t>(cap);
        vals_alt = cv.take<uint32_t>(cap);
        sort_tmp = cv.take<char>(sort_bytes);
        cell_start = cv.take<int32_t>(ncells + 2);
        rec = cv.take<double>((size_t)6 * (size_t)cap);
        krange = cv.take<int32_t>((size_t)2 * (size_t)cap);
        h_out = cv.take<double>(host ? out_len : 0);                  // the host form's device copy
        values_copy = cv.take<double>(host_v ? std::max<int64_t>(c->n, 0) : 0);
        return cv.bytes;
    };
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    double *d_out = host ? h_out : out;
    const double *d_values = host_v ? values_copy : values;

    // ---- read-back 2: the particles that can reach a node ---------------------------------------------------------------
    int64_t nsel = 0;
    if (count > 0) {
        SPH_HIP(hipMemsetAsync(cursor, 0, sizeof(uint32_t), st));
        const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((s.n_slots + RB - 1) / RB, 4 * RB_MAX));
        cube_select<<<dim3(nb), dim3(RB), 0, st>>>(c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], s, fr, nd, g, keys, vals, cursor, cap);
        SPH_HIP(hipGetLastError());
        SPH_HIP(hipMemcpyAsync(c->rnd_pinned + 16, cursor, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));
        nsel = std::min<int64_t>(*reinterpret_cast<const uint32_t *>(c->rnd_pinned + 16), cap);
    }

    if (nsel == 0) {
        SPH_HIP(hipMemsetAsync(d_out, 0, (size_t)out_len * sizeof(double), st));
    } else {
        unsigned cbits = 1;
        while (cbits < 32 && ((int64_t)1 << cbits) < ncells) cbits++;
        size_t tmp = sort_bytes;
        SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, keys, keys_alt, vals, vals_alt, (size_t)nsel, 0u, 32u + cbits, st));
        start_table<<<dim3((unsigned)((ncells + 1 + 255) / 256)), dim3(256), 0, st>>>(keys_alt, nsel, ncells, cell_start);
        if (host_v) SPH_HIP(hipMemcpyAsync(values_copy, values, (size_t)c->n * sizeof(double), hipMemcpyHostToDevice, st));
        Fields f{c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], c->f[SPH_F_VX], c->f[SPH_F_VY], c->f[SPH_F_VZ], c->f[SPH_F_M],
                 c->f[SPH_F_C], d_values};
        cube_records<<<dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, st>>>(f, s, fr, ch, vals_alt, nsel, rec, krange, cap);
        SPH_HIP(hipGetLastError());
        GatherArgs a{};
        a.nd = nd; a.g = g; a.ch = ch; a.reach = reach;
        a.pu = rec; a.pv = rec + cap; a.vl = rec + 2 * cap; a.y0 = rec + 3 * cap; a.ih = rec + 4 * cap; a.sg = rec + 5 * cap;
        a.klo = krange; a.khi = krange + cap;
        a.cell_start = cell_start;
        a.per_velocity = (d->flags & SPH_CUBE_PER_VELOCITY) != 0;
        a.tiles_v = (nd.n[1] + TV - 1) / TV;
        a.out = d_out;
        const int64_t tiles = (int64_t)((nd.n[0] + TU - 1) / TU) * a.tiles_v;
        const int chunks = (d->n_chan + CC - 1) / CC;
        if (tiles > 0x7fffffff || chunks > 65535) return arg_error(c, who, "too many image nodes or channels");
        cube_gather<<<dim3((unsigned)tiles, (unsigned)chunks), dim3(GT), 0, st>>>(a);
        SPH_HIP(hipGetLastError());
    }
    if (host) {
        SPH_HIP(hipMemcpyAsync(out, d_out, (size_t)out_len * sizeof(double), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));
    }
    return SPH_OK;
}

}  // namespace sph
