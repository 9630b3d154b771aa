// transfer.hip -- sph_transfer: emission-absorption images of the owned gas seen along any direction: intensity, optical
// depth, transmission and the depth of the tau = tau_surface surface.
//
// Every image node composites the particles whose footprint covers it front to back (include/summersph.h, "emission-
// absorption images", has the definition): the order of the terms matters, so the pass sorts by depth and every tile of
// nodes walks a depth-ordered list.  Not part of the step loop: nothing here reads or writes the context's grid, cell
// table, neighbour list, statistics or flags.
//
// Pipeline (all on ctx->stream, the analysis calls' scratch):
//   transfer_stats_partial, stats_final  owned gas inside the clip box: max h, min h, count, bad K or S       (read-back 1)
//   transfer_count                 the selected particles that reach a node and the tiles they touch: sizes   (read-back 2)
//   transfer_select                the same particles -> (id, slot), compacted with an atomic cursor
//   rocprim radix sort             by id, then transfer_depth_keys and a stable sort by the sortable image of D_j: (D, id)
//   transfer_records               in depth order: SoA records {P_u, P_v, D, y0 = m kappa / (pi h^2), 1 / h, S} and the
//                                  number of tiles of 8 x 8 nodes the particle touches (the nodes within its reach, a box)
//   rocprim exclusive scan, transfer_emit   one entry (tile << 32 | depth rank) per particle and tile, in rank order
//   rocprim radix sort             stable, on the tile bits alone: every tile's entries stay in depth order
//   start_table                    tile start table
//   transfer_gather                one wavefront per tile, lane = node.  The tile's records are staged into LDS 128 at a
//                                  time in list order.  Per record a ballot gives the nodes inside its footprint; the
//                                  (record, node) pairs of a segment are then evaluated 64 at a time (F, one expm1: the
//                                  cost of the pass, at full lane occupancy however few nodes a record covers) and
//                                  applied per node in list order.  The loop ends with the list or when no lane runs.
// A node's value is therefore a function of the descriptor, the selected particles and their ids alone: bitwise
// reproducible and independent of the context's sorted order.
// The selection, the h rule, the reach, the nodes, the frame and start_table are image_common.hpp's, shared with render.hip
// and cube.hip.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>

#include "image_common.hpp"
#include "spline_column.hpp"

// the definition fixes the order of the frame's sums and of the compositing; no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int RB = 256;            // reduction / select block
constexpr int RB_MAX = 1024;       // blocks of the reduction
constexpr int NSTAT = 4, NMIN = 0, NMAX = 2;       // max h, max(-h); count, particles with a bad K or S
constexpr int TU = 8, TV = 8;      // image nodes per tile (v fastest)
constexpr int GT = TU * TV;        // threads per gather workgroup: one wavefront, lane = node
static_assert(GT == WAVE, "transfer_gather ballots over the nodes of one wavefront");
#ifndef TRANSFER_STAGE
#define TRANSFER_STAGE 128         // A/B switch ("Emission-absorption images"): records per LDS stage
#endif
constexpr int CH = TRANSFER_STAGE; // 6 planes of doubles: 6 KB
#ifndef TRANSFER_PAIRS
#define TRANSFER_PAIRS 256         // A/B switch: (record, node) pairs evaluated per segment of a stage (18 bytes each)
#endif
constexpr int PC = TRANSFER_PAIRS;
constexpr int PSKIP = 0x8000;
static_assert(PC >= GT && CH * GT <= PSKIP, "a record's 64 pairs fit a segment; (record << 6 | lane) stays below the skip bit");
constexpr int64_t MAX_ENTRIES = (int64_t)1 << 31;

// where K or S of a slot comes from: a field of the context (slot order), the caller's array (original order) or 1
struct Src {
    const double *field, *values;
};

__device__ __forceinline__ double src_at(const Src &s, const int32_t *orig, int64_t i) {
    return s.field ? s.field[i] : (s.values ? s.values[orig[i]] : 1.0);
}

// the tiles [t0[a], t1[a]] that hold the nodes within the reach of P; false: none
__device__ __forceinline__ bool tile_range(const Nodes<2> &nd, double pu, double pv, double reach, int t0[2], int t1[2]) {
    int i0, i1;
    if (!node_range(nd, 0, pu, reach, i0, i1)) return false;
    t0[0] = i0 / TU; t1[0] = i1 / TU;
    if (!node_range(nd, 1, pv, reach, i0, i1)) return false;
    t0[1] = i0 / TV; t1[1] = i1 / TV;
    return true;
}

// partial[b * NSTAT + k]: max h, max -h, count, bad K or S over block b's grid-stride share of the selection
__global__ __launch_bounds__(RB) void transfer_stats_partial(const double *__restrict__ x, const double *__restrict__ y,
                                                             const double *__restrict__ z, Sel s, Src K, Src S,
                                                             double *__restrict__ partial) {
    double v[NSTAT] = {-INFINITY, -INFINITY, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < s.n_slots; i += (int64_t)gridDim.x * RB) {
        if (!selected(s, i, x[i], y[i], z[i])) continue;
        const double h = sel_h(s, i);
        v[0] = fmax(v[0], h);
        v[1] = fmax(v[1], -h);
        v[2] += 1.0;
        const double k = src_at(K, s.orig, i), sj = src_at(S, s.orig, i);
        if (!(k >= 0.0 && k < INFINITY) || !(fabs(sj) < INFINITY)) v[3] += 1.0;
    }
    stats_block_partial<NMIN, NMAX, RB>(v, partial);
}

// the selected particles that reach a node: P_uv and the tiles; false for every other slot
__device__ __forceinline__ bool reaches(const Sel &s, const Frame &fr, const Nodes<2> &nd, int64_t i, double px, double py,
                                        double pz, int t0[2], int t1[2]) {
    if (!selected(s, i, px, py, pz)) return false;
    const double dx = px - fr.centre[0], dy = py - fr.centre[1], dz = pz - fr.centre[2];
    const double reach = sel_reach(s, i);
    return tile_range(nd, row_dot(fr.rot, 0, dx, dy, dz), row_dot(fr.rot, 1, dx, dy, dz), reach, t0, t1);
}

// sizes[0]: particles that reach a node, sizes[1]: entries (particle, tile)
__global__ __launch_bounds__(RB) void transfer_count(const double *__restrict__ x, const double *__restrict__ y,
                                                     const double *__restrict__ z, Sel s, Frame fr, Nodes<2> nd,
                                                     unsigned long long *__restrict__ sizes) {
    unsigned long long np = 0, ne = 0;
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < s.n_slots; i += (int64_t)gridDim.x * RB) {
        int t0[2], t1[2];
        if (!reaches(s, fr, nd, i, x[i], y[i], z[i], t0, t1)) continue;
        np += 1;
        ne += (unsigned long long)(t1[0] - t0[0] + 1) * (unsigned long long)(t1[1] - t0[1] + 1);
    }
    __shared__ unsigned long long sm[2][RB / WAVE];
    for (int o = 32; o > 0; o >>= 1) {
        np += __shfl_xor(np, o, 64);
        ne += __shfl_xor(ne, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = np; sm[1][threadIdx.x >> 6] = ne; }
    __syncthreads();
    if (threadIdx.x < 2) {                                     // integer sums: exact in any order, one atomic a block
        unsigned long long r = 0;
        for (int w = 0; w < RB / WAVE; w++) r += sm[threadIdx.x][w];
        if (r > 0) atomicAdd(&sizes[threadIdx.x], r);
    }
}

// the same particles -> (original id, slot)
__global__ __launch_bounds__(RB) void transfer_select(const double *__restrict__ x, const double *__restrict__ y,
                                                      const double *__restrict__ z, Sel s, Frame fr, Nodes<2> nd,
                                                      uint32_t *__restrict__ ids, uint32_t *__restrict__ slots,
                                                      uint32_t *__restrict__ cursor, int64_t cap) {
    for (int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x; i < s.n_slots; i += (int64_t)gridDim.x * RB) {
        int t0[2], t1[2];
        if (!reaches(s, fr, nd, i, x[i], y[i], z[i], t0, t1)) continue;
        const uint32_t k = atomicAdd(cursor, 1u);
        if ((int64_t)k < cap) {
            ids[k] = (uint32_t)s.orig[i];
            slots[k] = (uint32_t)i;
        }
    }
}

// the sortable image of D_j: unsigned order = the order of the doubles, -0.0 and +0.0 the same key
__global__ __launch_bounds__(256) void transfer_depth_keys(const double *__restrict__ x, const double *__restrict__ y,
                                                           const double *__restrict__ z, Frame fr,
                                                           const uint32_t *__restrict__ slots, int64_t n,
                                                           uint64_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t j = slots[i];
    const double D = row_dot(fr.rot, 2, x[j] - fr.centre[0], y[j] - fr.centre[1], z[j] - fr.centre[2]) + 0.0;    // -0.0 -> +0.0
    const uint64_t b = (uint64_t)__double_as_longlong(D);
    keys[i] = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct Fields {
    const double *x, *y, *z, *m;
};

// records in depth order: P_u, P_v, D, y0 = m kappa / (pi h^2), 1 / h, S; cnt[i]: the tiles particle i touches
__global__ __launch_bounds__(256) void transfer_records(Fields f, Sel s, Frame fr, Nodes<2> nd, Src K, Src S, double kappa_scale,
                                                        const uint32_t *__restrict__ slots, int64_t n,
                                                        double *__restrict__ rec, int64_t stride, uint32_t *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { cnt[i] = 0; return; }                                // the scan's last element: the total
    const int64_t j = slots[i];
    const double h = sel_h(s, j);
    const double dx = f.x[j] - fr.centre[0], dy = f.y[j] - fr.centre[1], dz = f.z[j] - fr.centre[2];
    const double pu = row_dot(fr.rot, 0, dx, dy, dz), pv = row_dot(fr.rot, 1, dx, dy, dz);
    const double kappa = kappa_scale * src_at(K, s.orig, j);
    rec[i] = pu;
    rec[stride + i] = pv;
    rec[2 * stride + i] = row_dot(fr.rot, 2, dx, dy, dz);
    rec[3 * stride + i] = (f.m[j] * kappa) / (M_PI * (h * h));
    rec[4 * stride + i] = 1.0 / h;
    rec[5 * stride + i] = src_at(S, s.orig, j);
    int t0[2], t1[2];
    const bool any = tile_range(nd, pu, pv, reach_of(h), t0, t1);
    cnt[i] = any ? (uint32_t)(t1[0] - t0[0] + 1) * (uint32_t)(t1[1] - t0[1] + 1) : 0u;
}

// entries (tile << 32 | depth rank) of particle i at off[i] ..: rank order, a particle's tiles ascending
__global__ __launch_bounds__(256) void transfer_emit(const double *__restrict__ rec, int64_t stride, Sel s, Nodes<2> nd,
                                                     int32_t tiles_v, const uint32_t *__restrict__ slots,
                                                     const uint32_t *__restrict__ off, int64_t n, int64_t cap,
                                                     uint64_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double reach = sel_reach(s, slots[i]);
    int t0[2], t1[2];
    if (!tile_range(nd, rec[i], rec[stride + i], reach, t0, t1)) return;     // transfer_records' test
    int64_t o = off[i];
    const int64_t end = min((int64_t)off[i + 1], cap);
    for (int tu = t0[0]; tu <= t1[0]; tu++)
        for (int tv = t0[1]; tv <= t1[1]; tv++, o++)
            if (o < end) keys[o] = ((uint64_t)((int64_t)tu * tiles_v + tv) << 32) | (uint64_t)i;
}

struct GatherArgs {
    Nodes<2> nd;
    const double *pu, *pv, *dp, *y0, *ih, *sf;
    const uint64_t *entries;       // (tile << 32 | depth rank), tile-major, a tile's in depth order
    const int32_t *tile_start;     // null: no particle reaches a node
    double tau_surface, tau_max, background;
    int32_t tiles_v;               // tiles along v
    uint32_t n_rec;                // records
    double *out;
};

// blockIdx.x: tile of TU x TV nodes, lane = node.  A stage of records is worked off in segments of at most PC (record,
// node) pairs, three steps each: (1) per record, every lane tests its node and a ballot gives the record's mask of nodes;
// the pairs are numbered in (record, lane) order; (2) the 64 lanes evaluate F and expm1 of 64 pairs at a time -- the
// expensive part, which does not depend on the state of a node, at full lane occupancy however few nodes a record covers;
// (3) per record again, the lanes in its mask fetch their pair's dtau and a and make the update.  Every pair is computed
// from its node's and its record's values by the same operations and every node meets its pairs in list order, so the
// result is that of evaluating them one record at a time.
__global__ __launch_bounds__(GT) void transfer_gather(GatherArgs A) {
    __shared__ double su[CH], sv[CH], sd[CH], sy0[CH], sih[CH], ss[CH];
    __shared__ double ncu[GT], ncv[GT];
    __shared__ uint64_t smask[CH];
    __shared__ int32_t sbase[CH];
    __shared__ double pdt[PC], pa[PC];
    __shared__ uint16_t ppair[PC];                             // record of the stage << 6 | lane; PSKIP: p >= 2

    const Nodes<2> &nd = A.nd;
    const int t = threadIdx.x;
    const int tu = blockIdx.x / A.tiles_v, tv = blockIdx.x % A.tiles_v;
    const int iu = tu * TU + t / TV, iv = tv * TV + t % TV;
    const bool valid = iu < nd.n[0] && iv < nd.n[1];
    const double cu = node_coord(nd, 0, min(iu, nd.n[0] - 1)), cv = node_coord(nd, 1, min(iv, nd.n[1] - 1));
    const uint64_t below = ((uint64_t)1 << t) - 1;             // the lanes before this one
    ncu[t] = cu;
    ncv[t] = cv;

    double tau = 0.0, T = 1.0, I = 0.0, surf = NAN;
    bool running = valid;
    const int beg = A.tile_start ? A.tile_start[blockIdx.x] : 0, end = A.tile_start ? A.tile_start[blockIdx.x + 1] : 0;
    for (int cb = beg; cb < end; cb += CH) {
        if (__ballot(running) == 0) break;                     // every node of the tile is opaque
        const int cnt = min(CH, end - cb);
        __syncthreads();                                       // the previous stage has been read
        for (int e = t; e < cnt; e += GT) {
            const uint32_t r = min((uint32_t)A.entries[cb + e], A.n_rec - 1);
            su[e] = A.pu[r]; sv[e] = A.pv[r]; sd[e] = A.dp[r]; sy0[e] = A.y0[r]; sih[e] = A.ih[r]; ss[e] = A.sf[r];
        }
        __syncthreads();
        for (int js = 0; js < cnt;) {
            // (1) the pairs of the records js .. je - 1: every lane reads the same record (an LDS broadcast)
            int np = 0, je = js;
            for (; je < cnt; je++) {
                const double du = cu - su[je], dv = cv - sv[je];
                const double ih = sih[je];
                const bool hit = running && (du * du + dv * dv) * (ih * ih) <= 4.0000001;     // beyond it p > 2
                const uint64_t m = __ballot(hit);
                const int c = __popcll(m);
                if (np + c > PC) break;                        // a record has at most 64 pairs <= PC: je > js
                if (t == 0) { smask[je] = m; sbase[je] = np; }
                if (hit) ppair[np + __popcll(m & below)] = (uint16_t)((je << 6) | t);
                np += c;
            }
            __syncthreads();
            // (2) dtau and a = -expm1(-dtau) of every pair
            for (int q = t; q < np; q += GT) {
                const int e = ppair[q], j = e >> 6, l = e & 63;
                const double du = ncu[l] - su[j], dv = ncv[l] - sv[j];
                const double p = sqrt(du * du + dv * dv) * sih[j];
                if (p < 2.0) {
                    const double dtau = sy0[j] * spline_column(p);
                    pdt[q] = dtau;
                    pa[q] = -expm1(-dtau);
                } else {
                    ppair[q] = (uint16_t)(e | PSKIP);          // the particle is skipped at this node
                }
            }
            __syncthreads();
            // (3) the updates, record by record
            for (int j = js; j < je; j++) {
                const uint64_t m = smask[j];
                if (m == 0) continue;
                if (running && ((m >> t) & 1)) {
                    const int q = sbase[j] + __popcll(m & below);
                    if (!(ppair[q] & PSKIP)) {
                        const double dtau = pdt[q], a = pa[q];
                        I = I + (ss[j] * T) * a;
                        T = T - T * a;
                        tau = tau + dtau;
                        if (surf != surf && tau >= A.tau_surface) surf = sd[j];
                        if (tau >= A.tau_max) running = false;
                    }
                }
            }
            __syncthreads();                                   // the pairs have been read
            js = je;
        }
    }
    if (valid) {
        const int64_t plane = (int64_t)nd.n[0] * nd.n[1];
        const int64_t o = (int64_t)iu * nd.n[1] + iv;
        A.out[o] = I + T * A.background;
        A.out[plane + o] = tau;
        A.out[2 * plane + o] = T;
        A.out[3 * plane + o] = surf;
    }
}

bool selector_ok(int32_t id) { return id == SPH_TRANSFER_VALUES || id == SPH_TRANSFER_ONE || (id >= 0 && id < SPH_F_COUNT); }

}  // namespace

int transfer_run(sph_ctx *c, const sph_transfer_desc *d, const double *source, const double *kappa, double *out,
                 int64_t out_len, bool host) {
    const char *who = "sph_transfer";
    if (!d || !out) return arg_error(c, who, "null descriptor or output");
    if (d->reserved != 0) return arg_error(c, who, "reserved must be 0");
    if (d->flags != 0) return arg_error(c, who, "unknown flags");
    if (d->n_u < 1 || d->n_v < 1) return arg_error(c, who, "n_u and n_v must be >= 1");
    const int64_t pixels = (int64_t)d->n_u * d->n_v;
    if (pixels > ((int64_t)1 << 38)) return arg_error(c, who, "too many image nodes");
    if (out_len != 4 * pixels) return arg_error(c, who, "out_len does not match 4 n_u n_v");
    if (!(d->h >= 0.0) || !std::isfinite(d->h)) return arg_error(c, who, "h must be finite and >= 0");
    for (int a = 0; a < 2; a++)
        if (!(d->lo[a] <= d->hi[a]) || !std::isfinite(d->lo[a]) || !std::isfinite(d->hi[a])) return arg_error(c, who, "lo > hi");
    for (int a = 0; a < 3; a++) {
        if (std::isnan(d->clip_lo[a]) || std::isnan(d->clip_hi[a])) return arg_error(c, who, "NaN clip box");
        if (!std::isfinite(d->centre[a])) return arg_error(c, who, "centre must be finite");
    }
    if (!(d->kappa_scale >= 0.0) || !std::isfinite(d->kappa_scale)) return arg_error(c, who, "kappa_scale must be finite and >= 0");
    if (!(d->tau_surface > 0.0)) return arg_error(c, who, "tau_surface must be > 0");
    if (!(d->tau_max > 0.0)) return arg_error(c, who, "tau_max must be > 0");
    if (!std::isfinite(d->background)) return arg_error(c, who, "background must be finite");
    if (!selector_ok(d->source) || !selector_ok(d->kappa)) return arg_error(c, who, "source or kappa selector out of range");
    if ((d->source == SPH_TRANSFER_VALUES) != (source != nullptr))
        return arg_error(c, who, "source must be given with SPH_TRANSFER_VALUES and only then");
    if ((d->kappa == SPH_TRANSFER_VALUES) != (kappa != nullptr))
        return arg_error(c, who, "kappa must be given with SPH_TRANSFER_VALUES and only then");
    if (!check_rot(d->rot)) return arg_error(c, who, "rot must be orthonormal and right-handed within 1e-12");
    for (int32_t id : {d->source, d->kappa})
        if (id >= 0 && !field_ready(*c, c->variable, id)) {
            c->err = "sph_transfer: a field named by source or kappa is stale (sph_download_field would refuse it)";
            return SPH_ERR_STATE;
        }
    const int64_t tiles_u = ((int64_t)d->n_u + TU - 1) / TU, tiles_v = ((int64_t)d->n_v + TV - 1) / TV;
    const int64_t ntiles = tiles_u * tiles_v;
    if (ntiles > 0x7fffffff) return arg_error(c, who, "too many image nodes");

    hipStream_t st = c->stream;
    const Sel s = make_sel(c, d->clip_lo, d->clip_hi, d->h);
    Frame fr{};
    for (int a = 0; a < 3; a++) fr.centre[a] = d->centre[a];
    for (int a = 0; a < 9; a++) fr.rot[a] = d->rot[a];
    const int32_t n_uv[2] = {d->n_u, d->n_v};
    const Nodes<2> nd = make_nodes<2>(d->lo, d->hi, n_uv);

    SPH_TRY(analysis_pinned(c));
    // ---- scratch.  It is sized three times (the statistics; the particles; the entries) and may move when it grows: what
    //      has to survive a growth is the host form's copies of the caller's arrays, which are then staged again -------------
    const int64_t n_vals = std::max<int64_t>(c->n, 0);
    const bool copy_s = host && source, copy_k = host && kappa;
    double *partial, *stats, *s_copy, *k_copy, *h_out;
    unsigned long long *sizes;
    uint32_t *cursor;
    auto head = [&](Carve &cv) {
        partial = cv.take<double>((size_t)RB_MAX * NSTAT);
        stats = cv.take<double>(NSTAT + 1);
        sizes = cv.take<unsigned long long>(2);
        cursor = cv.take<uint32_t>(1);
        s_copy = cv.take<double>(copy_s ? n_vals : 0);
        k_copy = cv.take<double>(copy_k ? n_vals : 0);
        h_out = cv.take<double>(host ? out_len : 0);               // the host form's device copy
    };
    char *buf = nullptr;
    auto stage_values = [&]() -> int {
        if (copy_s && n_vals > 0) SPH_HIP(hipMemcpyAsync(s_copy, source, (size_t)n_vals * sizeof(double), hipMemcpyHostToDevice, st));
        if (copy_k && n_vals > 0) SPH_HIP(hipMemcpyAsync(k_copy, kappa, (size_t)n_vals * sizeof(double), hipMemcpyHostToDevice, st));
        return SPH_OK;
    };
    {
        Carve cv{};
        head(cv);
        SPH_TRY(analysis_scratch(c, cv.bytes, &buf));
        cv = Carve{buf};
        head(cv);
        SPH_TRY(stage_values());
    }
    auto src_of = [&](int32_t id, const double *copy, const double *given) {
        Src r{};
        if (id >= 0) r.field = c->f[id];
        else if (id == SPH_TRANSFER_VALUES) r.values = host ? copy : given;
        return r;
    };
    Src K = src_of(d->kappa, k_copy, kappa), S = src_of(d->source, s_copy, source);

    // ---- read-back 1: the selection's h range, its size and its bad inputs -------------------------------------------------
    double hs[NSTAT] = {-INFINITY, -INFINITY, 0.0, 0.0};
    if (s.n_slots > 0) {
        const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((s.n_slots + RB - 1) / RB, RB_MAX));
        transfer_stats_partial<<<dim3(nb), dim3(RB), 0, st>>>(c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], s, K, S, partial);
        SPH_TRY((stats_read_back<NSTAT, NMIN, NMAX>(c, partial, nb, stats, hs)));
    }
    const int64_t count = (int64_t)hs[2];
    const double h_max = hs[0], h_min = -hs[1];
    SPH_TRY(check_h_range(c, who, count, h_max, h_min));
    if (hs[3] > 0.0) return arg_error(c, who, "a selected particle has a negative or non-finite K or a non-finite S");

    // ---- read-back 2: the particles that reach a node and the entries of the tile lists -----------------------------------
    int64_t nsel = 0, nent = 0;
    const int nb_sel = (int)std::max<int64_t>(1, std::min<int64_t>((s.n_slots + RB - 1) / RB, 4 * RB_MAX));
    if (count > 0) {
        SPH_HIP(hipMemsetAsync(sizes, 0, 2 * sizeof(unsigned long long), st));
        const int nb_cnt = std::min(nb_sel, RB_MAX);
        transfer_count<<<dim3(nb_cnt), dim3(RB), 0, st>>>(c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], s, fr, nd, sizes);
        SPH_HIP(hipGetLastError());
        SPH_HIP(hipMemcpyAsync(c->rnd_pinned + 16, sizes, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));
        const unsigned long long *back = reinterpret_cast<const unsigned long long *>(c->rnd_pinned + 16);
        if (back[1] >= (unsigned long long)MAX_ENTRIES) {
            c->err = "sph_transfer: 2^31 or more tile-list entries (a large h over a small image extent)";
            return SPH_ERR_NOMEM;
        }
        nsel = (int64_t)back[0];
        nent = (int64_t)back[1];
    }

    GatherArgs a{};
    a.nd = nd;
    a.tau_surface = d->tau_surface; a.tau_max = d->tau_max; a.background = d->background;
    a.tiles_v = (int32_t)tiles_v;
    if (nsel == 0) {
        a.out = host ? h_out : out;
    } else {
        // ---- scratch, the rest --------------------------------------------------------------------------------------------
        const int64_t cap = nsel, ecap = std::max<int64_t>(nent, 1);
        unsigned tbits = 1;
        while (tbits < 31 && ((int64_t)1 << tbits) < ntiles) tbits++;
        size_t sort_ids = 0, sort_depth = 0, sort_tiles = 0, scan_bytes = 0;
        SPH_HIP(rocprim::radix_sort_pairs(nullptr, sort_ids, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                          (uint32_t *)nullptr, (size_t)cap, 0u, 32u, st));
        SPH_HIP(rocprim::radix_sort_pairs(nullptr, sort_depth, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                          (uint32_t *)nullptr, (size_t)cap, 0u, 64u, st));
        SPH_HIP(rocprim::radix_sort_keys(nullptr, sort_tiles, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)ecap, 32u,
                                         32u + tbits, st));
        SPH_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)(cap + 1),
                                        rocprim::plus<uint32_t>(), st));
        const size_t tmp_bytes = std::max(std::max(sort_ids, sort_depth), std::max(sort_tiles, scan_bytes));
        uint32_t *ids, *ids_alt, *slots, *slots_alt, *slots_d, *cnt, *off;
        uint64_t *dkeys, *dkeys_alt, *ent, *ent_alt;
        char *tmp;
        int32_t *tile_start;
        double *rec;
        auto layout = [&](Carve cv) {
            head(cv);
            ids = cv.take<uint32_t>(cap);
            ids_alt = cv.take<uint32_t>(cap);
            slots = cv.take<uint32_t>(cap);
            slots_alt = cv.take<uint32_t>(cap);
            slots_d = cv.take<uint32_t>(cap);
            dkeys = cv.take<uint64_t>(cap);
            dkeys_alt = cv.take<uint64_t>(cap);
            cnt = cv.take<uint32_t>(cap + 1);
            off = cv.take<uint32_t>(cap + 1);
            rec = cv.take<double>((size_t)6 * (size_t)cap);
            ent = cv.take<uint64_t>(ecap);
            ent_alt = cv.take<uint64_t>(ecap);
            tile_start = cv.take<int32_t>(ntiles + 2);
            tmp = cv.take<char>(tmp_bytes);
            return cv.bytes;
        };
        const size_t before = c->rnd_bytes;
        SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
        layout(Carve{buf});
        if (c->rnd_bytes != before) SPH_TRY(stage_values());          // the scratch moved
        K = src_of(d->kappa, k_copy, kappa);
        S = src_of(d->source, s_copy, source);
        a.out = host ? h_out : out;

        const double *x = c->f[SPH_F_X], *y = c->f[SPH_F_Y], *z = c->f[SPH_F_Z];
        SPH_HIP(hipMemsetAsync(cursor, 0, sizeof(uint32_t), st));
        transfer_select<<<dim3(nb_sel), dim3(RB), 0, st>>>(x, y, z, s, fr, nd, ids, slots, cursor, cap);
        SPH_HIP(hipGetLastError());
        // (D, id): by id, then stably by depth
        size_t tb = tmp_bytes;
        SPH_HIP(rocprim::radix_sort_pairs(tmp, tb, ids, ids_alt, slots, slots_alt, (size_t)nsel, 0u, 32u, st));
        const unsigned gb = (unsigned)((nsel + 1 + 255) / 256);
        transfer_depth_keys<<<dim3(gb), dim3(256), 0, st>>>(x, y, z, fr, slots_alt, nsel, dkeys);
        SPH_HIP(hipGetLastError());
        tb = tmp_bytes;
        SPH_HIP(rocprim::radix_sort_pairs(tmp, tb, dkeys, dkeys_alt, slots_alt, slots_d, (size_t)nsel, 0u, 64u, st));
        Fields f{x, y, z, c->f[SPH_F_M]};
        transfer_records<<<dim3(gb), dim3(256), 0, st>>>(f, s, fr, nd, K, S, d->kappa_scale, slots_d, nsel, rec, cap, cnt);
        SPH_HIP(hipGetLastError());
        tb = tmp_bytes;
        SPH_HIP(rocprim::exclusive_scan(tmp, tb, cnt, off, 0u, (size_t)(nsel + 1), rocprim::plus<uint32_t>(), st));
        if (nent > 0) {
            transfer_emit<<<dim3(gb), dim3(256), 0, st>>>(rec, cap, s, nd, (int32_t)tiles_v, slots_d, off, nsel, nent, ent);
            SPH_HIP(hipGetLastError());
            tb = tmp_bytes;
            SPH_HIP(rocprim::radix_sort_keys(tmp, tb, ent, ent_alt, (size_t)nent, 32u, 32u + tbits, st));
        }
        start_table<<<dim3((unsigned)((ntiles + 1 + 255) / 256)), dim3(256), 0, st>>>(ent_alt, nent, ntiles, tile_start);
        SPH_HIP(hipGetLastError());
        a.pu = rec; a.pv = rec + cap; a.dp = rec + 2 * cap; a.y0 = rec + 3 * cap; a.ih = rec + 4 * cap; a.sf = rec + 5 * cap;
        a.entries = ent_alt;
        a.tile_start = tile_start;
        a.n_rec = (uint32_t)nsel;
    }
    transfer_gather<<<dim3((unsigned)ntiles), dim3(GT), 0, st>>>(a);
    SPH_HIP(hipGetLastError());
    if (host) {
        SPH_HIP(hipMemcpyAsync(out, a.out, (size_t)out_len * sizeof(double), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));
    }
    return SPH_OK;
}

}  // namespace sph
