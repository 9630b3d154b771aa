// modes.hip -- the azimuthal Fourier sums C_m, S_m of a weight per ring and the logarithmic-spiral sums over (m, p) of the
// whole annulus, in sph_profile's disc frame (include/summersph.h, sph_modes).
//
// Not part of the step loop: nothing here reads or writes the context's grid, cell table, neighbour list, statistics or
// flags.  The scratch is the one the analysis calls share (analysis_scratch).
//
// Every sum is accumulated exactly (exact_sum.hpp): a term is formed in double in the header's order, scaled by the power of
// two that the largest weight fixes, rounded to a 64-bit integer and added into a 128-bit integer.  Integer addition is
// associative, so the order of the records, the LDS histograms' copies, the per-block slabs and the launch change no bit.
//
// Pipeline (all on ctx->stream; the exponent and the counts stay on the device):
//   modes_select   every slot: frame position (disc_frame.hpp), selection, weight; a usable selected particle's record
//                  {c, s, u, w, ring} is appended to a compact list (one integer atomic per wavefront; the list's order is
//                  free because the sums are exact); the ring from a search of the edge table in LDS; per-block partials of
//                  max |w| and the four counts
//   modes_head     one wavefront: the partials -> Info: the exponent e, counts[4]
//   modes_rings    persistent blocks, lanes are records: the recurrence (c + i s)^m and one add per term into an LDS integer
//                  histogram {lo, hi} per (ring, sum) in up to MAX_COPIES copies dealt by lane; rings in chunks where the
//                  histogram does not fit; one slab per block, plain stores
//   modes_spiral   the transposed pass: a tile of records {c, s, u, w} in LDS, every lane one p[l] and its 2 (m_max + 1)
//                  accumulators in registers; every lane reads the same record (an LDS broadcast), takes sincos(p[l] u) once
//                  and runs the recurrence; one slab per (block, wavefront share), plain stores
//   modes_sum      one wavefront per accumulator adds the slabs: the raw limbs and the ring counts
//   modes_convert  device form only: limbs -> correctly rounded doubles, e and the counts to the caller's memory (the host
//                  form calls sph_modes_finish's code)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "disc_frame.hpp"
#include "exact_sum.hpp"
#include "reduce_common.hpp"

// every term in one documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int KB = 256;                    // block of every kernel here (modes_spiral: at most)
constexpr int SEL_BLOCKS = 1024;           // select blocks at most (grid-stride beyond)
constexpr int MAX_M = SPH_MODES_MAX_M;
constexpr int MAX_RINGS = SPH_MODES_MAX_RINGS;
constexpr int MAX_P = SPH_MODES_MAX_P;
constexpr int RING_BLOCKS = 512;           // persistent blocks of modes_rings at most
constexpr int SPIRAL_BLOCKS = 1024;        // ... of modes_spiral
constexpr int TILE = 256;                  // records of modes_spiral's LDS tile (8 KB)
constexpr int NST = 5;                     // statistics of modes_select: max |w|, then counts[4]

struct Sel {
    const double *x, *y, *z, *m, *q;       // q null: A = 1
    const double *edge;                    // n_r + 1 (device)
    double r_min, r_max, z_max, r_ref;
    int32_t n_r, weight_m, q_by_id, spiral;
};

struct Rec {                               // the compact list, n_slots entries each
    double *c, *s, *u, *w;                 // u: log(R / r_ref); NaN where R == 0 (not in the spiral sums)
    int32_t *k;                            // ring
};

struct Info {
    int64_t counts[4];                     // the header's counts
    int32_t exp;                           // e
    int32_t n_list;                        // records appended (modes_select); zeroed before the launch
};

// A wavefront's records take consecutive list entries through one integer atomic.  (One atomic per block and round brings
// the kernel from 186 to 26 us at 10^6 particles, but the block's rendezvous costs scalar registers the kernel does not
// have: 8 to 29 of them spill.  DESIGN section 29.)
__global__ __launch_bounds__(KB) void modes_select(const int32_t *__restrict__ orig, int64_t n_slots, int64_t n_owned, DiscFrame f,
                                                   Sel s, Rec r, Info *__restrict__ info, double *__restrict__ part) {
    __shared__ double edge[MAX_RINGS + 1];
    for (int k = threadIdx.x; k <= s.n_r; k += KB) edge[k] = s.edge[k];
    __syncthreads();
    double c0[3], cv[3], cm;
    centre_of(f, c0, cv, cm);
    double v[NST];
#pragma unroll
    for (int k = 0; k < NST; k++) v[k] = stat_identity<0, 1>(k);
    const int lane = threadIdx.x & 63;
    for (int64_t i0 = (int64_t)blockIdx.x * KB; i0 < n_slots; i0 += (int64_t)gridDim.x * KB) {   // uniform over the block
        const int64_t i = i0 + threadIdx.x;
        bool sel = false;
        double c = 1.0, sn = 0.0, u = 0.0, w = 0.0;
        int ring = 0;
        const int32_t id = i < n_slots ? orig[i] : -1;
        if (id >= 0 && id < n_owned) {                    // ghosts and replaced ghosts are not selected
            const double px = s.x[i], py = s.y[i], pz = s.z[i];
            if (!(finite(px) && finite(py) && finite(pz))) {
                v[3] += 1.0;
            } else {
                const Pos p = frame_pos(f, c0, px, py, pz);
                if (!(p.R >= s.r_min && p.R < s.r_max && fabs(p.Z) < s.z_max)) {
                    v[2] += 1.0;
                } else {
                    const double base = s.weight_m ? s.m[i] : 1.0;
                    const double a = s.q ? s.q[s.q_by_id ? (int64_t)id : i] : 1.0;
                    if (!(finite(base) && finite(a))) {
                        v[3] += 1.0;
                    } else {
                        sel = true;
                        w = base * a;
                        if (p.R > 0.0) {
                            c = p.X / p.R;
                            sn = p.Y / p.R;
                            if (s.spiral) u = log(p.R / s.r_ref);
                        } else {
                            u = NAN;                      // the mark that keeps it out of the spiral sums
                            v[4] += 1.0;
                        }
                        int lo = 0, up = s.n_r - 1;       // the last ring with edge[k] <= R
                        while (lo < up) {
                            const int mid = (lo + up + 1) >> 1;
                            if (edge[mid] <= p.R) lo = mid; else up = mid - 1;
                        }
                        ring = lo;
                        v[0] = fmax(v[0], fabs(w));
                        v[1] += 1.0;
                    }
                }
            }
        }
        const uint64_t sm = __ballot(sel);
        if (sm != 0) {
            const int leader = __ffsll((unsigned long long)sm) - 1;
            int32_t at = 0;
            if (lane == leader) at = atomicAdd(&info->n_list, (int32_t)__popcll(sm));
            at = __shfl(at, leader, 64);
            if (sel) {
                const int64_t j = at + __popcll(sm & (((uint64_t)1 << lane) - 1));
                r.c[j] = c; r.s[j] = sn; r.u[j] = u; r.w[j] = w; r.k[j] = ring;
            }
        }
    }
    stats_block_partial<0, 1, KB, NST>(v, part);
}

// one wavefront: the partials -> the exponent and the counts
__global__ __launch_bounds__(WAVE) void modes_head(const double *__restrict__ part, int nb, Info *__restrict__ info) {
    const int lane = threadIdx.x;
    double v[NST];
#pragma unroll
    for (int k = 0; k < NST; k++) v[k] = stat_identity<0, 1>(k);
    for (int b = lane; b < nb; b += WAVE)
#pragma unroll
        for (int k = 0; k < NST; k++) v[k] = stat_join<0, 1>(k, v[k], part[b * NST + k]);
#pragma unroll
    for (int k = 0; k < NST; k++) v[k] = stat_wave<0, 1>(k, v[k]);
    if (lane != 0) return;
    info->exp = exp_above(2.0 * fmax(v[0], 0.0));         // B = 2 W_max; nothing selected: W_max = 0
#pragma unroll
    for (int k = 0; k < 4; k++) info->counts[k] = (int64_t)v[1 + k];
}

struct RingArgs {
    Rec rec;
    const Info *info;
    unsigned long long *slab;              // gridDim.x slabs of n_r na {lo, hi}, na = 1 + 2 (m_max + 1): count, C_0 S_0 C_1 ..
    int32_t n_r, m_max;
    int32_t chunk, copies;                 // rings a block's histogram holds at a time, and how many copies of them
};

// lanes are records; the rings in chunks of a.chunk (one chunk unless n_r na > HIST: the pass then runs once per chunk and
// keeps the records of the chunk's rings)
__global__ __launch_bounds__(KB) void modes_rings(RingArgs a) {
    __shared__ unsigned long long hist[2 * HIST];
    const int n_r = a.n_r, m_max = a.m_max, na = 2 * (m_max + 1) + 1;
    const int64_t n = a.info->n_list;
    const int sh = 62 - a.info->exp;
    for (int k0 = 0; k0 < n_r; k0 += a.chunk) {
        const int k1 = min(n_r, k0 + a.chunk);
        const int acc = (k1 - k0) * na;                  // accumulators of one copy: acc copies <= HIST
        unsigned long long *mine = hist_mine(hist, a.copies, acc);
        __syncthreads();                                 // the last chunk's flush is done
        hist_zero(hist, a.copies, acc, KB);
        __syncthreads();
        for (int64_t j = (int64_t)blockIdx.x * KB + threadIdx.x; j < n; j += (int64_t)gridDim.x * KB) {
            const int k = a.rec.k[j];
            if (k < k0 || k >= k1) continue;
            const double c = a.rec.c[j], s = a.rec.s[j], w = a.rec.w[j];
            unsigned long long *h = mine + 2 * (k - k0) * na;
            atomicAdd(h, 1ull);
            double cm = 1.0, sm = 0.0;
            for (int m = 0; m <= m_max; m++) {
                add_term(h + 2 * (1 + 2 * m), w * cm, sh);
                if (m) add_term(h + 2 * (2 + 2 * m), w * sm, sh);        // s_0 = 0: nothing to add
                const double cn = cm * c - sm * s, sn = sm * c + cm * s;
                cm = cn;
                sm = sn;
            }
        }
        __syncthreads();
        hist_flush(hist, a.copies, acc, KB, a.slab + 2 * ((size_t)blockIdx.x * n_r + k0) * na);
    }
}

struct SpiralArgs {
    Rec rec;
    const Info *info;
    const double *p;                       // n_p (device)
    unsigned long long *slab;              // gridDim.x nsub slabs of (m_max + 1) n_p 2 {lo, hi}
    int32_t n_p, ng, nsub;                 // ng = wavefronts that cover the p table; nsub = shares of a tile's records
};

// blockDim.x = 64 ng nsub.  Wavefront v: the p's 64 (v % ng) + lane, the tile's records v / ng, v / ng + nsub, ...
template <int M1>
__global__ __launch_bounds__(KB) void modes_spiral(SpiralArgs a) {
    __shared__ double tc[TILE], ts[TILE], tu[TILE], tw[TILE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int l = 64 * (wv % a.ng) + lane, sub = wv / a.ng;
    const double p = l < a.n_p ? a.p[l] : 0.0;
    const int64_t n = a.info->n_list;
    const int sh = 62 - a.info->exp;
    unsigned long long lo[2 * M1], hi[2 * M1];
#pragma unroll
    for (int k = 0; k < 2 * M1; k++) lo[k] = hi[k] = 0ull;
    for (int64_t t0 = (int64_t)blockIdx.x * TILE; t0 < n; t0 += (int64_t)gridDim.x * TILE) {
        const int cnt = (int)min((int64_t)TILE, n - t0);
        __syncthreads();                                 // the last tile has been read
        for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
            const double u = a.rec.u[t0 + j];
            const bool centre = u != u;                  // R == 0: weight 0 here, every term an exact 0
            tc[j] = a.rec.c[t0 + j];
            ts[j] = a.rec.s[t0 + j];
            tu[j] = centre ? 0.0 : u;
            tw[j] = centre ? 0.0 : a.rec.w[t0 + j];
        }
        __syncthreads();
        for (int j = sub; j < cnt; j += a.nsub) {
            const double c = tc[j], s = ts[j], w = tw[j];          // every lane the same address: broadcasts
            const double th = p * tu[j];
            double sp, cp;
            sincos(th, &sp, &cp);
            double cm = 1.0, sm = 0.0;
#pragma unroll
            for (int m = 0; m < M1; m++) {
                add_fixed(lo[2 * m], hi[2 * m], to_fixed(w * (cm * cp - sm * sp), sh));
                add_fixed(lo[2 * m + 1], hi[2 * m + 1], to_fixed(w * (sm * cp + cm * sp), sh));
                const double cn = cm * c - sm * s, sn = sm * c + cm * s;
                cm = cn;
                sm = sn;
            }
        }
    }
    if (l >= a.n_p) return;
    unsigned long long *out = a.slab + 2 * ((size_t)blockIdx.x * a.nsub + sub) * ((size_t)M1 * a.n_p * 2);
#pragma unroll
    for (int m = 0; m < M1; m++) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const size_t g = ((size_t)m * a.n_p + l) * 2 + t;
            out[2 * g] = lo[2 * m + t];
            out[2 * g + 1] = hi[2 * m + t];
        }
    }
}

// the sum of the slabs' accumulators g, g in [0, n_acc): one wavefront per accumulator (slab_sum).  na == 0: raw[g] (the
// spiral block).  na > 0: the ring slabs' layout, accumulator 0 of every na the ring's count and the others the ring block's
// sums in order
__global__ __launch_bounds__(KB) void modes_sum(const unsigned long long *__restrict__ slab, int nslab, int64_t n_acc, int na,
                                                unsigned long long *__restrict__ raw, int64_t *__restrict__ ring_counts) {
    const int64_t g = (int64_t)blockIdx.x * (KB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_acc) return;
    unsigned long long lo, hi;
    slab_sum(slab, nslab, n_acc, g, lane, lo, hi);
    if (lane != 0) return;
    int64_t o = g;
    if (na > 0) {
        const int64_t k = g / na, j = g % na;
        if (j == 0) {
            ring_counts[k] = (int64_t)lo;
            return;
        }
        o = k * (na - 1) + (j - 1);
    }
    raw[2 * o] = lo;
    raw[2 * o + 1] = hi;
}

__global__ __launch_bounds__(KB) void modes_convert(const unsigned long long *__restrict__ raw, const Info *__restrict__ info,
                                                    int64_t n_acc, double *__restrict__ sums, int32_t *__restrict__ exp,
                                                    int64_t *__restrict__ counts) {
    const int64_t g = (int64_t)blockIdx.x * KB + threadIdx.x;
    if (g == 0) {
        if (exp) exp[0] = info->exp;
        if (counts)
            for (int k = 0; k < 4; k++) counts[k] = info->counts[k];
    }
    if (g >= n_acc) return;
    sums[g] = limbs_to_double(raw[2 * g], raw[2 * g + 1], info->exp);
}

int64_t n_acc_of(const sph_modes_desc *d) { return 2 * (int64_t)(d->m_max + 1) * ((int64_t)d->n_r + d->n_p); }

// the checks that need no context; null: fine
const char *check_desc(const sph_modes_desc *d) {
    for (int k = 0; k < 3; k++)
        if (d->reserved[k] != 0) return "reserved must be 0";
    if (d->flags & ~SPH_MODES_LOG) return "unknown flags";
    if (d->weight != SPH_MODES_W_ONE && d->weight != SPH_MODES_W_MASS) return "unknown weight";
    if (d->n_r < 1 || d->n_r > MAX_RINGS) return "n_r must be 1 .. SPH_MODES_MAX_RINGS";
    if (d->m_max < 0 || d->m_max > MAX_M) return "m_max must be 0 .. SPH_MODES_MAX_M";
    if (d->n_p < 0 || d->n_p > MAX_P) return "n_p must be 0 .. SPH_MODES_MAX_P";
    if (d->n_q < 0 || d->n_q > 1) return "n_q must be 0 or 1";
    if (d->n_rows < 0 || d->n_rows > MAX_ROWS) return "n_rows must be 0 .. 16";
    if (d->n_q == 1 && !source_ok(d->q, d->n_rows)) return "the quantity source is neither an SPH_F_* id nor a row below n_rows";
    if (!std::isfinite(d->r_min) || !std::isfinite(d->r_max) || d->r_min < 0.0 || !(d->r_min < d->r_max))
        return "need finite 0 <= r_min < r_max";
    if ((d->flags & SPH_MODES_LOG) && d->r_min == 0.0) return "SPH_MODES_LOG needs r_min > 0";
    if (std::isnan(d->z_max)) return "z_max is NaN";
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(d->normal[a])) return "the normal is not finite";
    if (d->normal[0] == 0.0 && d->normal[1] == 0.0 && d->normal[2] == 0.0) return "the normal is zero";
    if (d->sink < -1) return "sink out of range";
    if (d->sink < 0)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(d->centre[a]) || !std::isfinite(d->centre_v[a])) return "the centre is not finite";
    if (d->n_p > 0) {
        if (!std::isfinite(d->r_ref) || !(d->r_ref > 0.0)) return "the spiral sums need a finite r_ref > 0";
        if (!std::isfinite(d->p_min) || !std::isfinite(d->p_max)) return "the p range is not finite";
        if (d->p_min > d->p_max) return "p_min > p_max";
    }
    return nullptr;
}

// edge[k], k in [0, n_r], and p[l], l in [0, n_p) (either may be null).  null: fine
const char *make_tables(const sph_modes_desc *d, double *edge, double *p) {
    if (edge) {
        ring_edge_table(d->r_min, d->r_max, d->n_r, (d->flags & SPH_MODES_LOG) != 0, edge);
        for (int k = 0; k < d->n_r; k++)
            if (!(edge[k] < edge[k + 1])) return "ring edges are not strictly increasing (rings too narrow)";
    }
    if (p) {
        const int np = d->n_p;
        for (int l = 0; l < np; l++) {
            p[l] = np == 1 ? d->p_min : d->p_min + ((double)l * (d->p_max - d->p_min)) / (double)(np - 1);
            if (!std::isfinite(p[l])) return "the p table is not finite";
        }
    }
    return nullptr;
}

template <int M1>
void launch_spiral(unsigned nblk, unsigned threads, hipStream_t st, const SpiralArgs &a) {
    modes_spiral<M1><<<dim3(nblk), dim3(threads), 0, st>>>(a);
}

}  // namespace

int modes_run(sph_ctx *c, const sph_modes_desc *d, const double *values, double *sums, int64_t n_out, uint64_t *raw, int32_t *exp,
              int64_t *ring_counts, int64_t *counts, bool host) {
    const char *who = "sph_modes";
    if (!d) return arg_error(c, who, "null descriptor");
    if (!sums) return arg_error(c, who, "null output");
    if (const char *why = check_desc(d)) return arg_error(c, who, why);
    if (d->sink >= c->ns) return arg_error(c, who, "sink out of range");
    const int n_r = d->n_r, m1 = d->m_max + 1, n_p = d->n_p;
    const int64_t n_acc = n_acc_of(d), n_ring = 2 * (int64_t)m1 * n_r, n_spiral = n_acc - n_ring;
    if (n_out != n_acc) return arg_error(c, who, "n_out != 2 (m_max + 1) (n_r + n_p)");
    if ((d->n_rows == 0) != (values == nullptr)) return arg_error(c, who, "values must be given with n_rows > 0 and only then");
    DiscFrame f{};
    if (!frame_axes(d->normal, f.n, f.e1, f.e2)) return arg_error(c, who, "the normal cannot be normalised");

    // the two tables travel in the stream's order from a pinned staging copy (sph_profile's), rewritten only once its last
    // upload is done
    hipStream_t st = c->stream;
    const size_t ne = (size_t)n_r + 1, nt = ne + (size_t)n_p;
    double *tables = nullptr;
    SPH_TRY(table_staging(c, nt, &tables));
    if (const char *why = make_tables(d, tables, tables + ne)) return arg_error(c, who, why);

    const bool by_row = d->n_q == 1 && d->q < 0;
    if (d->n_q == 1 && d->q >= 0 && !field_ready(*c, c->variable, d->q)) {
        c->err = "sph_modes: a field is stale (as sph_download_field would refuse it)";
        return SPH_ERR_STATE;
    }

    const int64_t n = c->n, n_slots = c->cap > 0 ? c->n_slots : 0;
    if (n_slots == 0 || n == 0) {                        // nothing held: zero sums, e = 0
        SPH_HIP(zero_output(sums, (size_t)n_acc, host, st));
        SPH_HIP(zero_output(raw, (size_t)n_acc * 2, host, st));
        SPH_HIP(zero_output(exp, 1, host, st));
        SPH_HIP(zero_output(ring_counts, (size_t)n_r, host, st));
        SPH_HIP(zero_output(counts, 4, host, st));
        return SPH_OK;
    }

    // modes_rings: the histogram's chunking and the slabs
    const int na = 2 * m1 + 1;
    const int64_t n_acc_r = (int64_t)n_r * na;
    const HistPlan hp = hist_plan<2 * (MAX_M + 1) + 1>(n_r, na, std::min<int64_t>(RING_BLOCKS, (n_slots + KB - 1) / KB));
    const int nblk_r = hp.nslab;
    // modes_spiral: ng wavefronts cover the p table, the other wavefronts of a block share a tile's records
    const int ng = n_p > 0 ? (n_p + WAVE - 1) / WAVE : 1;
    const int nsub = std::max(1, (KB / WAVE) / ng);
    const int64_t slab_s = n_spiral;                     // accumulators of a spiral slab
    const int nblk_s = n_p > 0 ? (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)SPIRAL_BLOCKS,
                                                                             (int64_t)(SLAB_BYTES / ((size_t)slab_s * 16 * nsub)),
                                                                             (n_slots + TILE - 1) / TILE}))
                               : 0;
    const int nb = (int)std::min<int64_t>((n_slots + KB - 1) / KB, SEL_BLOCKS);
    Rec rec{};
    double *d_tables, *part, *h_values;
    unsigned long long *slab_ring, *slab_spiral, *blk;
    auto layout = [&](Carve cv) {
        rec.c = cv.take<double>(n_slots);
        rec.s = cv.take<double>(n_slots);
        rec.u = cv.take<double>(n_slots);
        rec.w = cv.take<double>(n_slots);
        rec.k = cv.take<int32_t>(n_slots);
        d_tables = cv.take<double>(nt);
        part = cv.take<double>((size_t)NST * (size_t)nb);
        slab_ring = cv.take<unsigned long long>((size_t)nblk_r * (size_t)n_acc_r * 2);
        slab_spiral = cv.take<unsigned long long>((size_t)nblk_s * (size_t)nsub * (size_t)slab_s * 2);
        // what the host form reads back in one copy: the limbs, the ring counts, Info
        blk = cv.take<unsigned long long>((size_t)n_acc * 2 + (size_t)n_r + sizeof(Info) / sizeof(unsigned long long));
        h_values = cv.take<double>(host && by_row ? (size_t)n : 0);             // the host form's device copy of the row
        return cv.bytes;
    };
    static_assert(sizeof(Info) % sizeof(unsigned long long) == 0, "Info is read back as 64-bit words");
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    unsigned long long *d_raw = raw && !host ? reinterpret_cast<unsigned long long *>(raw) : blk;
    int64_t *d_rc = ring_counts && !host ? ring_counts : reinterpret_cast<int64_t *>(blk + (size_t)n_acc * 2);
    Info *info = reinterpret_cast<Info *>(blk + (size_t)n_acc * 2 + (size_t)n_r);
    const double *q_ptr = nullptr;
    if (d->n_q == 1) {
        if (!by_row) {
            q_ptr = c->f[d->q];
        } else {
            const size_t row = (size_t)(-1 - d->q) * (size_t)n;
            if (host) {
                SPH_HIP(hipMemcpyAsync(h_values, values + row, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
                q_ptr = h_values;
            } else {
                q_ptr = values + row;
            }
        }
    }
    SPH_HIP(hipMemcpyAsync(d_tables, tables, nt * sizeof(double), hipMemcpyHostToDevice, st));
    SPH_HIP(hipEventRecord(c->prf_evt, st));
    SPH_HIP(hipMemsetAsync(info, 0, sizeof(Info), st));

    for (int a = 0; a < 3; a++) { f.c[a] = d->centre[a]; f.cv[a] = d->centre_v[a]; }
    f.sink = c->sink;
    f.sink_k = d->sink;
    Sel s{};
    s.x = c->f[SPH_F_X]; s.y = c->f[SPH_F_Y]; s.z = c->f[SPH_F_Z];
    s.m = c->f[SPH_F_M];
    s.q = q_ptr;
    s.edge = d_tables;
    s.r_min = d->r_min; s.r_max = d->r_max; s.z_max = d->z_max; s.r_ref = d->r_ref;
    s.n_r = n_r;
    s.weight_m = d->weight == SPH_MODES_W_MASS;
    s.q_by_id = by_row;
    s.spiral = n_p > 0;

    modes_select<<<dim3((unsigned)nb), dim3(KB), 0, st>>>(c->orig, n_slots, c->n_owned, f, s, rec, info, part);
    modes_head<<<dim3(1), dim3(WAVE), 0, st>>>(part, nb, info);
    RingArgs ra{rec, info, slab_ring, n_r, d->m_max, hp.chunk, hp.copies};
    modes_rings<<<dim3((unsigned)nblk_r), dim3(KB), 0, st>>>(ra);
    modes_sum<<<dim3(blocks(n_acc_r, KB / WAVE)), dim3(KB), 0, st>>>(slab_ring, nblk_r, n_acc_r, na, d_raw, d_rc);
    SPH_HIP(hipGetLastError());
    if (n_p > 0) {
        SpiralArgs sa{rec, info, d_tables + ne, slab_spiral, n_p, ng, nsub};
        const unsigned threads = (unsigned)(WAVE * ng * nsub);
        switch (m1) {
            case 1: launch_spiral<1>(nblk_s, threads, st, sa); break;
            case 2: launch_spiral<2>(nblk_s, threads, st, sa); break;
            case 3: launch_spiral<3>(nblk_s, threads, st, sa); break;
            case 4: launch_spiral<4>(nblk_s, threads, st, sa); break;
            case 5: launch_spiral<5>(nblk_s, threads, st, sa); break;
            case 6: launch_spiral<6>(nblk_s, threads, st, sa); break;
            case 7: launch_spiral<7>(nblk_s, threads, st, sa); break;
            case 8: launch_spiral<8>(nblk_s, threads, st, sa); break;
            default: launch_spiral<9>(nblk_s, threads, st, sa); break;
        }
        modes_sum<<<dim3(blocks(n_spiral, KB / WAVE)), dim3(KB), 0, st>>>(slab_spiral, nblk_s * nsub, n_spiral, 0, d_raw + 2 * n_ring,
                                                                         nullptr);
        SPH_HIP(hipGetLastError());
    }
    if (!host) {
        modes_convert<<<dim3(blocks(n_acc, KB)), dim3(KB), 0, st>>>(d_raw, info, n_acc, sums, exp, counts);
        SPH_HIP(hipGetLastError());
        return SPH_OK;
    }
    // host form: limbs, ring counts, exponent and counts in one read-back, then sph_modes_finish's conversion
    std::vector<uint64_t> h((size_t)n_acc * 2 + (size_t)n_r + sizeof(Info) / sizeof(uint64_t));
    SPH_HIP(hipMemcpyAsync(h.data(), blk, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    Info hi;
    std::memcpy(&hi, h.data() + (size_t)n_acc * 2 + (size_t)n_r, sizeof(Info));
    finish_all(h.data(), n_acc, &hi.exp, 1, sums);
    if (raw) std::memcpy(raw, h.data(), (size_t)n_acc * 2 * sizeof(uint64_t));
    if (exp) exp[0] = hi.exp;
    if (ring_counts) std::memcpy(ring_counts, h.data() + (size_t)n_acc * 2, (size_t)n_r * sizeof(int64_t));
    if (counts) std::memcpy(counts, hi.counts, 4 * sizeof(int64_t));
    return SPH_OK;
}

}  // namespace sph

extern "C" int sph_modes_tables(const sph_modes_desc *d, double *edges_out, double *p_out) {
    using namespace sph;
    if (!d) return SPH_ERR_ARG;
    if (check_desc(d)) return SPH_ERR_ARG;
    double n[3], e1[3], e2[3];
    if (!frame_axes(d->normal, n, e1, e2)) return SPH_ERR_ARG;
    std::vector<double> t((size_t)d->n_r + 1 + (size_t)d->n_p);
    if (make_tables(d, t.data(), t.data() + d->n_r + 1)) return SPH_ERR_ARG;
    if (edges_out) std::memcpy(edges_out, t.data(), ((size_t)d->n_r + 1) * sizeof(double));
    if (p_out && d->n_p > 0) std::memcpy(p_out, t.data() + d->n_r + 1, (size_t)d->n_p * sizeof(double));
    return SPH_OK;
}

extern "C" int sph_modes_finish(const sph_modes_desc *d, const int32_t *exp, const uint64_t *raw, double *sums) {
    using namespace sph;
    if (!d || !exp || !raw || !sums) return SPH_ERR_ARG;
    if (d->n_r < 1 || d->n_r > MAX_RINGS || d->m_max < 0 || d->m_max > MAX_M || d->n_p < 0 || d->n_p > MAX_P) return SPH_ERR_ARG;
    finish_all(raw, n_acc_of(d), exp, 1, sums);
    return SPH_OK;
}
