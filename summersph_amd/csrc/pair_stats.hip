// pair_stats.hip -- sums over the ordered pairs (i, j), j != i, of the owned gas binned by their separation r (or r / h_i):
// the pair-separation histogram g(r / h) and the structure functions of the velocity field and of any scalar
// (include/summersph.h, sph_pairs).  (pairs.hip is the step loop's pair passes; this is the analysis call.)
//
// Not part of the step loop: nothing here reads or writes the context's grid, cell table, neighbour list, statistics or
// flags.  The scratch is the one the analysis calls share (analysis_scratch).
//
// Every float sum is accumulated exactly: a term is formed in double in the header's order, scaled by a power of two that
// the sources' maxima fix, rounded to a 64-bit integer and added into a 128-bit integer.  Integer addition is associative,
// so the per-block LDS histograms, the per-block slabs and the order the targets are dealt in change no bit.
//
// Pipeline (all on ctx->stream; box, cell edge, maxima, exponents and counts stay on the device):
//   pairs_select   every slot: class (none / source / source and target) and the source's weight; per-block partials of the
//                  sources' box and maxima (w, |A_k|, |v|), the targets' h_max and the three counts
//   pairs_box      one wavefront: the partials -> Info: box, cell edge E = r_max (1 + 1e-6) (enlarged where an axis would
//                  need more than 2^21 - 8 cells), the exponent e_s of every sum, the counts
//   pairs_keys     every slot: the 63-bit cell key (cell_table.hpp) of a source, ~0 otherwise
//   rocprim radix sort (cell key, slot)
//   pairs_gather   sorted position p < n_src: the record {x y z vx vy vz w A_0..A_3 h} in sorted order; the first position
//                  of every cell enters the hash table; the targets' positions are appended to a list (one integer atomic
//                  per wavefront; the list's order is free because the sums are exact)
//   pairs_tails    the last position of every cell writes its end
//   pairs_bin      the hot kernel: persistent blocks, GL lanes per target, the 27 partner cells through the hash table,
//                  LDS integer histogram {lo, hi} per (bin, sum) in up to MAX_COPIES copies dealt by lane, added up and
//                  written out as one slab per block with plain stores
//   pairs_sum      one wavefront per (bin, sum) adds the slabs: the raw limbs
//   pairs_convert  device form only: limbs -> correctly rounded doubles (the host form calls sph_pairs_finish's code)
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cell_table.hpp"
#include "exact_sum.hpp"
#include "reduce_common.hpp"

// every term in one documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int KB = 256;                    // block of every kernel here
constexpr int BOX_BLOCKS = 1024;           // select blocks at most (grid-stride beyond)
constexpr int MAXQ = SPH_PAIRS_MAX_Q;
constexpr int MAXS = 2 + 2 * MAXQ + 4;     // sums per bin at most
constexpr int MAX_BINS = SPH_PAIRS_MAX_BINS;
constexpr int RS = 12;                     // doubles per sorted record: x y z vx vy vz w A0 A1 A2 A3 h
constexpr int GL = 8;                      // lanes per target
constexpr int BIN_BLOCKS = 512;            // persistent blocks of pairs_bin at most
constexpr int NST = 16;                    // statistics of pairs_select: 3 minima, 10 maxima, 3 counts
constexpr int ALL_FLAGS = SPH_PAIRS_LOG | SPH_PAIRS_EDGES | SPH_PAIRS_SCALE_H | SPH_PAIRS_VELOCITY;

struct Spec {
    const double *x, *y, *z, *vx, *vy, *vz, *m, *hf;
    const double *q[MAXQ];
    double clip_lo[3], clip_hi[3];
    double fixed_h, r_top;                 // r_top = edge[n_bins]
    uint32_t q_by_id;                      // bit k: q[k] is a row of values (by original id)
    int32_t n_q, weight_m, velocity, scale_h, stride, phase;
};

struct Info {
    double lo[3], inv_e, cut2;             // the sources' box, 1 / cell edge, the square of the cell edge
    int64_t n_tgt, n_src, n_bad;           // counts[3]
    int32_t exps[MAXS + 2];                // e_s per sum (exps[0] = 62: N is a plain count)
    int32_t n_list, pad;                   // targets appended so far (pairs_gather)
};

// class of every slot (0 none, 1 source, 3 source and target), its weight, the per-block partials
__global__ __launch_bounds__(KB) void pairs_select(const int32_t *__restrict__ orig, int64_t n_slots, int64_t n_owned, Spec s,
                                                   uint8_t *__restrict__ cls, double *__restrict__ part) {
    double v[NST];
#pragma unroll
    for (int k = 0; k < NST; k++) v[k] = stat_identity<3, 10>(k);
    for (int64_t i = (int64_t)blockIdx.x * KB + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * KB) {
        const int32_t id = orig[i];
        uint8_t c = 0;
        if (id >= 0 && id < n_owned) {                    // ghosts and replaced ghosts are neither source nor target
            const double px = s.x[i], py = s.y[i], pz = s.z[i];
            bool ok = finite(px) && finite(py) && finite(pz);
            double w = 1.0, h = 1.0, vm = 0.0, a[MAXQ];
            if (s.weight_m) { w = s.m[i]; ok = ok && finite(w); }
            if (s.scale_h) { h = s.hf ? s.hf[i] : s.fixed_h; ok = ok && finite(h) && h > 0.0; }
            if (s.velocity) {
                const double ux = s.vx[i], uy = s.vy[i], uz = s.vz[i];
                ok = ok && finite(ux) && finite(uy) && finite(uz);
                vm = fmax(fmax(fabs(ux), fabs(uy)), fabs(uz));
            }
#pragma unroll
            for (int k = 0; k < MAXQ; k++) {
                a[k] = 0.0;
                if (k < s.n_q) {
                    a[k] = s.q[k][(s.q_by_id >> k) & 1u ? (int64_t)id : i];
                    ok = ok && finite(a[k]);
                }
            }
            if (!ok) {
                v[15] += 1.0;
            } else {
                c = 1;
                v[0] = fmin(v[0], px); v[1] = fmin(v[1], py); v[2] = fmin(v[2], pz);
                v[3] = fmax(v[3], px); v[4] = fmax(v[4], py); v[5] = fmax(v[5], pz);
                v[6] = fmax(v[6], fabs(w));
#pragma unroll
                for (int k = 0; k < MAXQ; k++) v[7 + k] = fmax(v[7 + k], fabs(a[k]));
                v[11] = fmax(v[11], vm);
                v[14] += 1.0;
                const bool tgt = s.clip_lo[0] < px && px < s.clip_hi[0] && s.clip_lo[1] < py && py < s.clip_hi[1] &&
                                 s.clip_lo[2] < pz && pz < s.clip_hi[2] && id % s.stride == s.phase;
                if (tgt) {
                    c = 3;
                    v[12] = fmax(v[12], h);
                    v[13] += 1.0;
                }
            }
        }
        cls[i] = c;
    }
    stats_block_partial<3, 10, KB, NST>(v, part);
}

// one wavefront: the partials -> Info
__global__ __launch_bounds__(WAVE) void pairs_box(const double *__restrict__ part, int nb, Spec s, Info *__restrict__ info) {
    const int lane = threadIdx.x;
    double v[NST];
#pragma unroll
    for (int k = 0; k < NST; k++) v[k] = stat_identity<3, 10>(k);
    for (int b = lane; b < nb; b += WAVE)
#pragma unroll
        for (int k = 0; k < NST; k++) v[k] = stat_join<3, 10>(k, v[k], part[b * NST + k]);
#pragma unroll
    for (int k = 0; k < NST; k++) v[k] = stat_wave<3, 10>(k, v[k]);
    if (lane != 0) return;
#pragma unroll
    for (int k = 6; k < 13; k++) v[k] = fmax(v[k], 0.0);          // no source (no target): the maxima are 0
    const int64_t n_src = (int64_t)v[14], n_tgt = (int64_t)v[13];
    double e = (s.scale_h ? s.r_top * v[12] : s.r_top) * (1.0 + 1e-6);
    if (!(e > 0.0) || !finite(e) || n_src == 0 || n_tgt == 0) e = 1.0;          // nothing can be selected
    for (int a = 0; a < 3; a++) {
        const double ext = n_src > 0 ? v[3 + a] - v[a] : 0.0;
        if (ext / e > AXIS_CELLS) e = (ext / AXIS_CELLS) * (1.0 + 1e-6);
        info->lo[a] = n_src > 0 ? v[a] : 0.0;
    }
    info->inv_e = 1.0 / e;
    info->cut2 = e * e;
    info->n_tgt = n_tgt;
    info->n_src = n_src;
    info->n_bad = (int64_t)v[15];
    info->n_list = 0;
    info->pad = 0;
    // the bounds B_s (summersph.h, "Bounds") and their exponents
    const double w2 = v[6] * v[6], V = 4.0 * v[11];
    const int nq = s.n_q;
    info->exps[0] = 62;
    info->exps[1] = exp_above(w2);
#pragma unroll
    for (int k = 0; k < MAXQ; k++)
        if (k < nq) {
            const double A = 2.0 * v[7 + k];
            info->exps[2 + k] = exp_above(w2 * A);
            info->exps[2 + nq + k] = exp_above(w2 * (A * A));
        }
    if (s.velocity) {
        const double V2 = V * V;
        info->exps[2 + 2 * nq] = exp_above(w2 * V);
        info->exps[3 + 2 * nq] = exp_above(w2 * V2);
        info->exps[4 + 2 * nq] = exp_above(w2 * (V2 * V));
        info->exps[5 + 2 * nq] = exp_above(w2 * V2);
    }
}

__global__ __launch_bounds__(KB) void pairs_keys(const uint8_t *__restrict__ cls, int64_t n_slots, Spec s,
                                                 const Info *__restrict__ info, uint64_t *__restrict__ keys,
                                                 uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * KB + threadIdx.x;
    if (i >= n_slots) return;
    keys[i] = cls[i] ? cell_key(s.x[i], s.y[i], s.z[i], info->lo, info->inv_e) : ~0ull;
    vals[i] = (uint32_t)i;
}

// the records in sorted order, the table's starts, the target list
__global__ __launch_bounds__(KB) void pairs_gather(const int32_t *__restrict__ orig, const uint8_t *__restrict__ cls, Spec s,
                                                   const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sval,
                                                   Info *__restrict__ info, int64_t n_slots, double *__restrict__ rec,
                                                   int32_t *__restrict__ tlist, Ent *__restrict__ tab, uint64_t mask) {
    const int64_t p = (int64_t)blockIdx.x * KB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = p < n_slots && p < info->n_src;
    bool tgt = false;
    if (live) {
        const uint32_t i = sval[p];
        const int32_t id = orig[i];
        double *r = rec + p * RS;
        r[0] = s.x[i]; r[1] = s.y[i]; r[2] = s.z[i];
        r[3] = s.velocity ? s.vx[i] : 0.0; r[4] = s.velocity ? s.vy[i] : 0.0; r[5] = s.velocity ? s.vz[i] : 0.0;
        r[6] = s.weight_m ? s.m[i] : 1.0;
#pragma unroll
        for (int k = 0; k < MAXQ; k++) r[7 + k] = k < s.n_q ? s.q[k][(s.q_by_id >> k) & 1u ? (int64_t)id : (int64_t)i] : 0.0;
        r[11] = s.scale_h ? (s.hf ? s.hf[i] : s.fixed_h) : 1.0;
        tgt = cls[i] == 3;
        cell_enter(skey, p, tab, mask);
    }
    // the wavefront's targets take consecutive list entries: one integer atomic per wavefront
    const uint64_t tm = __ballot(tgt);
    if (tm == 0) return;
    const int leader = __ffsll((unsigned long long)tm) - 1;
    int32_t base = 0;
    if (lane == leader) base = atomicAdd(&info->n_list, (int32_t)__popcll(tm));
    base = __shfl(base, leader, 64);
    if (tgt) tlist[base + __popcll(tm & (((uint64_t)1 << lane) - 1))] = (int32_t)p;
}

__global__ __launch_bounds__(KB) void pairs_tails(const uint64_t *__restrict__ skey, const Info *__restrict__ info, int64_t n_slots,
                                                  Ent *__restrict__ tab, uint64_t mask) {
    cell_close(skey, (int64_t)blockIdx.x * KB + threadIdx.x, n_slots, info->n_src, tab, mask);
}

struct BinArgs {
    const double *rec;
    const uint64_t *skey;
    const int32_t *tlist;
    const Info *info;
    const Ent *tab;
    const double *edge;                    // n_bins + 1 (device)
    unsigned long long *slab;              // gridDim.x slabs of n_bins nsum {lo, hi}
    uint64_t mask;
    int32_t n_bins, n_q, nsum, scale_h;
    int32_t chunk, copies;                 // bins a block's histogram holds at a time, and how many copies of them
};

// GL lanes per target; the bins in chunks of a.chunk (one chunk unless n_bins nsum > HIST: the pair pass then runs once
// per chunk and keeps the pairs of the chunk's bins)
template <bool VEL, bool HASQ>
__global__ __launch_bounds__(KB) void pairs_bin(BinArgs a) {
    __shared__ double edge[MAX_BINS + 1];
    __shared__ unsigned long long hist[2 * HIST];
    const int n_bins = a.n_bins, nsum = a.nsum, nq = a.n_q;
    for (int k = threadIdx.x; k <= n_bins; k += KB) edge[k] = a.edge[k];
    const int sub = threadIdx.x % GL;
    const int64_t groups = (int64_t)gridDim.x * (KB / GL), g0 = (int64_t)blockIdx.x * (KB / GL) + threadIdx.x / GL;
    const int64_t n_tgt = a.info->n_list;
    const double cut2 = a.info->cut2;
    __shared__ int sh[MAXS];                             // 62 - e_s: in LDS, so that a runtime sum index costs no scratch
    if (threadIdx.x < MAXS) sh[threadIdx.x] = (int)threadIdx.x < nsum ? 62 - a.info->exps[threadIdx.x] : 0;
    for (int b0 = 0; b0 < n_bins; b0 += a.chunk) {
        const int b1 = min(n_bins, b0 + a.chunk);
        const int acc = (b1 - b0) * nsum;                // accumulators of one copy
        unsigned long long *mine = hist_mine(hist, a.copies, acc);
        __syncthreads();                                 // the edges are in; the last chunk's flush is done
        hist_zero(hist, a.copies, acc, KB);
        __syncthreads();
        const double e_lo = edge[b0], e_hi = edge[b1];
        for (int64_t t = g0; t < n_tgt; t += groups) {
            const int64_t p = a.tlist[t];
            const double *ri = a.rec + p * RS;
            const double xi = ri[0], yi = ri[1], zi = ri[2], wi = ri[6], hi = ri[11];
            double vi[3] = {0.0, 0.0, 0.0}, ai[MAXQ] = {0.0, 0.0, 0.0, 0.0};
            if (VEL) { vi[0] = ri[3]; vi[1] = ri[4]; vi[2] = ri[5]; }
            if (HASQ) {
#pragma unroll
                for (int k = 0; k < MAXQ; k++) ai[k] = ri[7 + k];
            }
            const uint64_t key = a.skey[p];
            const int64_t c0 = (int64_t)(key >> (2 * AXIS_BITS)), c1 = (int64_t)((key >> AXIS_BITS) & AXIS_MASK),
                          c2 = (int64_t)(key & AXIS_MASK);
            for (int o = 0; o < 27; o++) {
                const int64_t n0 = c0 + o / 9 - 1, n1 = c1 + (o / 3) % 3 - 1, n2 = c2 + o % 3 - 1;
                if (n0 < 0 || n1 < 0 || n2 < 0 || n0 > (int64_t)AXIS_MASK || n1 > (int64_t)AXIS_MASK || n2 > (int64_t)AXIS_MASK)
                    continue;
                const uint64_t nk = ((uint64_t)n0 << (2 * AXIS_BITS)) | ((uint64_t)n1 << AXIS_BITS) | (uint64_t)n2;
                const int64_t e = hash_slot(a.tab, a.mask, nk);
                if (e < 0) continue;
                const int64_t q1 = a.tab[e].end;
                for (int64_t q = (int64_t)a.tab[e].start + sub; q < q1; q += GL) {
                    if (q == p) continue;
                    const double *rj = a.rec + q * RS;
                    const double dx = rj[0] - xi, dy = rj[1] - yi, dz = rj[2] - zi;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 > cut2) continue;             // a selected pair has r < the cell edge: a filter only
                    const double r = sqrt(d2);
                    const double xv = a.scale_h ? r / hi : r;
                    if (!(xv >= e_lo && xv < e_hi)) continue;
                    int lo = b0, up = b1 - 1;            // the last bin with edge[k] <= xv
                    while (lo < up) {
                        const int mid = (lo + up + 1) >> 1;
                        if (edge[mid] <= xv) lo = mid; else up = mid - 1;
                    }
                    unsigned long long *h = mine + 2 * (lo - b0) * nsum;
                    const double w = wi * rj[6];
                    atomicAdd(h, 1ull);
                    add_term(h + 2, w, sh[1]);
                    if (HASQ) {
#pragma unroll
                        for (int k = 0; k < MAXQ; k++)
                            if (k < nq) {
                                const double dA = rj[7 + k] - ai[k];
                                add_term(h + 2 * (2 + k), w * dA, sh[2 + k]);
                                add_term(h + 2 * (2 + nq + k), w * (dA * dA), sh[2 + nq + k]);
                            }
                    }
                    if (VEL) {
                        const double ux = rj[3] - vi[0], uy = rj[4] - vi[1], uz = rj[5] - vi[2];
                        const double dot = (ux * dx + uy * dy) + uz * dz;
                        const double u = r == 0.0 ? 0.0 : dot / r;
                        const double u2 = u * u;
                        const int s0 = 2 + 2 * nq;
                        add_term(h + 2 * s0, w * u, sh[s0]);
                        add_term(h + 2 * (s0 + 1), w * u2, sh[s0 + 1]);
                        add_term(h + 2 * (s0 + 2), w * (u2 * u), sh[s0 + 2]);
                        add_term(h + 2 * (s0 + 3), w * ((ux * ux + uy * uy) + uz * uz), sh[s0 + 3]);
                    }
                }
            }
        }
        __syncthreads();
        hist_flush(hist, a.copies, acc, KB, a.slab + 2 * ((size_t)blockIdx.x * n_bins + b0) * nsum);
    }
}

// raw[g] = the sum of the slabs' accumulators g, g in [0, n_bins nsum): one wavefront per accumulator (slab_sum)
__global__ __launch_bounds__(KB) void pairs_sum(const unsigned long long *__restrict__ slab, int nblk, int64_t n_acc,
                                                unsigned long long *__restrict__ raw) {
    const int64_t g = (int64_t)blockIdx.x * (KB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_acc) return;
    unsigned long long lo, hi;
    slab_sum(slab, nblk, n_acc, g, lane, lo, hi);
    if (lane != 0) return;
    raw[2 * g] = lo;
    raw[2 * g + 1] = hi;
}

__global__ __launch_bounds__(KB) void pairs_convert(const unsigned long long *__restrict__ raw, const Info *__restrict__ info,
                                                    int nsum, int64_t n_acc, double *__restrict__ sums, int32_t *__restrict__ exps) {
    const int64_t g = (int64_t)blockIdx.x * KB + threadIdx.x;
    if (exps && g < nsum) exps[g] = info->exps[g];
    if (g >= n_acc) return;
    sums[g] = limbs_to_double(raw[2 * g], raw[2 * g + 1], info->exps[g % nsum]);
}

int nsum_of(const sph_pairs_desc *d) { return 2 + 2 * d->n_q + ((d->flags & SPH_PAIRS_VELOCITY) ? 4 : 0); }

// the checks that need no context and no table; null: fine
const char *check_desc(const sph_pairs_desc *d, const double *edges) {
    for (int k = 0; k < 3; k++)
        if (d->reserved[k] != 0) return "reserved must be 0";
    if (d->flags & ~ALL_FLAGS) return "unknown flags";
    if (d->weight != SPH_PAIRS_W_ONE && d->weight != SPH_PAIRS_W_MASS) return "unknown weight";
    if (d->n_bins < 1 || d->n_bins > MAX_BINS) return "n_bins must be 1 .. SPH_PAIRS_MAX_BINS";
    if (d->n_q < 0 || d->n_q > MAXQ) return "n_q must be 0 .. SPH_PAIRS_MAX_Q";
    if (d->n_rows < 0 || d->n_rows > MAX_ROWS) return "n_rows must be 0 .. 16";
    for (int k = 0; k < d->n_q; k++)
        if (!source_ok(d->q[k], d->n_rows)) return "a quantity source is neither an SPH_F_* id nor a row below n_rows";
    if (d->target_stride < 1) return "target_stride must be >= 1";
    if (d->target_phase < 0 || d->target_phase >= d->target_stride) return "target_phase must be 0 .. target_stride - 1";
    for (int a = 0; a < 3; a++)
        if (std::isnan(d->clip_lo[a]) || std::isnan(d->clip_hi[a])) return "the clip box has a NaN";
    const bool lg = (d->flags & SPH_PAIRS_LOG) != 0, ed = (d->flags & SPH_PAIRS_EDGES) != 0;
    if (lg && ed) return "LOG and EDGES together";
    if (ed != (edges != nullptr)) return "edges must be given with SPH_PAIRS_EDGES and only then";
    if (!ed) {
        if (!std::isfinite(d->lo) || !std::isfinite(d->hi) || !(d->lo < d->hi)) return "need finite lo < hi";
        if (lg && !(d->lo > 0.0)) return "logarithmic bins need lo > 0";
    }
    return nullptr;
}

// edge[k], k in [0, n]: sph_binned's formulas, or the caller's table.  null: fine
const char *make_edges(const sph_pairs_desc *d, const double *edges, double *edge) {
    const int n = d->n_bins;
    if (d->flags & SPH_PAIRS_EDGES) {
        std::memcpy(edge, edges, ((size_t)n + 1) * sizeof(double));
    } else {
        const bool lg = (d->flags & SPH_PAIRS_LOG) != 0;
        const double lo = d->lo, hi = d->hi;
        for (int k = 0; k < n; k++)
            edge[k] = lg ? lo * std::pow(hi / lo, (double)k / (double)n) : lo + ((double)k * (hi - lo)) / (double)n;
        edge[n] = hi;
    }
    for (int k = 0; k <= n; k++)
        if (!std::isfinite(edge[k])) return "an edge is not finite";
    for (int k = 0; k < n; k++)
        if (!(edge[k] < edge[k + 1])) return "the edges are not strictly increasing (bins too narrow)";
    return nullptr;
}

template <bool VEL, bool HASQ>
void launch_bin(unsigned nblk, hipStream_t st, const BinArgs &a) {
    pairs_bin<VEL, HASQ><<<dim3(nblk), dim3(KB), 0, st>>>(a);
}

}  // namespace

int pairs_run(sph_ctx *c, const sph_pairs_desc *d, const double *values, const double *edges, double *sums, int64_t n_out,
              uint64_t *raw, int32_t *exps, int64_t *counts, bool host) {
    const char *who = "sph_pairs";
    if (!d) return arg_error(c, who, "null descriptor");
    if (!sums) return arg_error(c, who, "null output");
    if (const char *why = check_desc(d, edges)) return arg_error(c, who, why);
    const int nq = d->n_q, nsum = nsum_of(d), n_bins = d->n_bins;
    const int64_t n_acc = (int64_t)n_bins * nsum;
    if (n_out != n_acc) return arg_error(c, who, "n_out != n_bins (2 + 2 n_q + 4 velocity)");
    if ((d->n_rows == 0) != (values == nullptr)) return arg_error(c, who, "values must be given with n_rows > 0 and only then");
    const bool scale_h = (d->flags & SPH_PAIRS_SCALE_H) != 0, velocity = (d->flags & SPH_PAIRS_VELOCITY) != 0;

    // the edge table travels in the stream's order from a pinned staging copy (sph_profile's), rewritten only once its
    // last upload is done
    hipStream_t st = c->stream;
    const size_t ne = (size_t)n_bins + 1;
    double *edge = nullptr;
    SPH_TRY(table_staging(c, ne, &edge));
    if (const char *why = make_edges(d, edges, edge)) return arg_error(c, who, why);

    uint32_t rows_used = 0;                              // the rows some quantity reads
    bool fresh = true;
    for (int k = 0; k < nq; k++) {
        if (d->q[k] < 0) rows_used |= 1u << (-1 - d->q[k]);
        else fresh = field_ready(*c, c->variable, d->q[k]) && fresh;
    }
    if (!fresh) {
        c->err = "sph_pairs: a field is stale (as sph_download_field would refuse it)";
        return SPH_ERR_STATE;
    }

    const int64_t n = c->n, n_slots = c->cap > 0 ? c->n_slots : 0;
    if (n_slots == 0 || n == 0) {                        // nothing held: zero sums
        SPH_HIP(zero_output(sums, (size_t)n_acc, host, st));
        SPH_HIP(zero_output(raw, (size_t)n_acc * 2, host, st));
        SPH_HIP(zero_output(exps, (size_t)nsum, host, st));
        SPH_HIP(zero_output(counts, 3, host, st));
        if (exps && host) exps[0] = 62;
        else if (exps) SPH_HIP(hipMemsetAsync(exps, 62, 1, st));            // little endian: the int32 62
        return SPH_OK;
    }

    const HistPlan hp = hist_plan<MAXS>(n_bins, nsum, BIN_BLOCKS);
    const int nblk = hp.nslab;
    const int nb = (int)std::min<int64_t>((n_slots + KB - 1) / KB, BOX_BLOCKS);
    int64_t tl = 1;
    while (tl < 2 * n_slots) tl <<= 1;                   // hash table: load <= 1/2
    size_t sort_bytes = 0;
    SPH_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)n_slots, 0u, 64u, st));
    uint64_t *keys, *keys_alt;
    uint32_t *vals, *vals_alt;
    char *sort_tmp;
    uint8_t *cls;
    double *d_edge, *rec, *part, *h_values, *h_sums;
    int32_t *tlist;
    Ent *tab;
    Info *info;
    unsigned long long *slab, *w_raw;
    auto layout = [&](Carve cv) {
        keys = cv.take<uint64_t>(n_slots);
        keys_alt = cv.take<uint64_t>(n_slots);
        vals = cv.take<uint32_t>(n_slots);
        vals_alt = cv.take<uint32_t>(n_slots);
        sort_tmp = cv.take<char>(sort_bytes);
        cls = cv.take<uint8_t>(n_slots);
        d_edge = cv.take<double>(ne);
        rec = cv.take<double>((size_t)RS * (size_t)n_slots);
        tlist = cv.take<int32_t>(n_slots);
        tab = cv.take<Ent>(tl);
        part = cv.take<double>((size_t)NST * (size_t)nb);
        info = cv.take<Info>(1);
        slab = cv.take<unsigned long long>((size_t)nblk * (size_t)n_acc * 2);
        w_raw = cv.take<unsigned long long>(raw && !host ? 0 : (size_t)n_acc * 2);       // where the caller gives no raw block
        h_values = cv.take<double>(host ? (size_t)d->n_rows * (size_t)n : 0);           // the host form's device copies
        h_sums = cv.take<double>(0);
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    (void)h_sums;
    unsigned long long *d_raw = raw && !host ? reinterpret_cast<unsigned long long *>(raw) : w_raw;
    const double *d_values = host ? h_values : values;
    if (host) {
        SPH_TRY(analysis_pinned(c));
        SPH_HIP(upload_rows(h_values, values, d->n_rows, rows_used, (size_t)n, st));
    }
    SPH_HIP(hipMemcpyAsync(d_edge, edge, ne * sizeof(double), hipMemcpyHostToDevice, st));
    SPH_HIP(hipEventRecord(c->prf_evt, st));

    Spec s{};
    s.x = c->f[SPH_F_X]; s.y = c->f[SPH_F_Y]; s.z = c->f[SPH_F_Z];
    s.vx = c->f[SPH_F_VX]; s.vy = c->f[SPH_F_VY]; s.vz = c->f[SPH_F_VZ];
    s.m = c->f[SPH_F_M];
    s.hf = c->variable ? c->f[SPH_F_H] : nullptr;
    for (int k = 0; k < nq; k++) {
        s.q[k] = d->q[k] >= 0 ? c->f[d->q[k]] : d_values + (size_t)(-1 - d->q[k]) * (size_t)n;
        if (d->q[k] < 0) s.q_by_id |= 1u << k;
    }
    for (int a = 0; a < 3; a++) { s.clip_lo[a] = d->clip_lo[a]; s.clip_hi[a] = d->clip_hi[a]; }
    s.fixed_h = c->p.h;
    s.r_top = edge[n_bins];
    s.n_q = nq;
    s.weight_m = d->weight == SPH_PAIRS_W_MASS;
    s.velocity = velocity;
    s.scale_h = scale_h;
    s.stride = d->target_stride;
    s.phase = d->target_phase;

    pairs_select<<<dim3((unsigned)nb), dim3(KB), 0, st>>>(c->orig, n_slots, c->n_owned, s, cls, part);
    pairs_box<<<dim3(1), dim3(WAVE), 0, st>>>(part, nb, s, info);
    pairs_keys<<<dim3(blocks(n_slots, KB)), dim3(KB), 0, st>>>(cls, n_slots, s, info, keys, vals);
    SPH_HIP(hipGetLastError());
    size_t tmp = sort_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, keys, keys_alt, vals, vals_alt, (size_t)n_slots, 0u, 64u, st));
    SPH_HIP(hipMemsetAsync(tab, 0xff, sizeof(Ent) * (size_t)tl, st));
    pairs_gather<<<dim3(blocks(n_slots, KB)), dim3(KB), 0, st>>>(c->orig, cls, s, keys_alt, vals_alt, info, n_slots, rec, tlist, tab,
                                                                 (uint64_t)(tl - 1));
    pairs_tails<<<dim3(blocks(n_slots, KB)), dim3(KB), 0, st>>>(keys_alt, info, n_slots, tab, (uint64_t)(tl - 1));
    BinArgs a{rec, keys_alt, tlist, info, tab, d_edge, slab, (uint64_t)(tl - 1), n_bins, nq, nsum, scale_h ? 1 : 0, hp.chunk, hp.copies};
    if (velocity) { if (nq) launch_bin<true, true>(nblk, st, a); else launch_bin<true, false>(nblk, st, a); }
    else { if (nq) launch_bin<false, true>(nblk, st, a); else launch_bin<false, false>(nblk, st, a); }
    pairs_sum<<<dim3(blocks(n_acc, KB / WAVE)), dim3(KB), 0, st>>>(slab, nblk, n_acc, d_raw);
    SPH_HIP(hipGetLastError());
    if (!host) {
        pairs_convert<<<dim3(blocks(std::max<int64_t>(n_acc, nsum), KB)), dim3(KB), 0, st>>>(d_raw, info, nsum, n_acc, sums, exps);
        SPH_HIP(hipGetLastError());
        if (counts) SPH_HIP(hipMemcpyAsync(counts, &info->n_tgt, 3 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        return SPH_OK;
    }
    // host form: limbs, exponents and counts in one read-back, then sph_pairs_finish's conversion
    std::vector<uint64_t> h_raw((size_t)n_acc * 2);
    Info *h_info = reinterpret_cast<Info *>(c->rnd_pinned);
    static_assert(sizeof(Info) <= 32 * sizeof(double), "Info must fit the analysis calls' pinned read-back slots");
    SPH_HIP(hipMemcpyAsync(h_info, info, sizeof(Info), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipMemcpyAsync(h_raw.data(), d_raw, h_raw.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    finish_all(h_raw.data(), n_acc, h_info->exps, nsum, sums);
    if (raw) std::memcpy(raw, h_raw.data(), h_raw.size() * sizeof(uint64_t));
    if (exps) std::memcpy(exps, h_info->exps, (size_t)nsum * sizeof(int32_t));
    if (counts) { counts[0] = h_info->n_tgt; counts[1] = h_info->n_src; counts[2] = h_info->n_bad; }
    return SPH_OK;
}

}  // namespace sph

extern "C" int sph_pairs_edges(const sph_pairs_desc *d, const double *edges, double *out) {
    using namespace sph;
    if (!d || !out) return SPH_ERR_ARG;
    if (check_desc(d, edges)) return SPH_ERR_ARG;
    std::vector<double> t((size_t)d->n_bins + 1);
    if (make_edges(d, edges, t.data())) return SPH_ERR_ARG;
    std::memcpy(out, t.data(), t.size() * sizeof(double));
    return SPH_OK;
}

extern "C" int sph_pairs_finish(const sph_pairs_desc *d, const int32_t *exps, const uint64_t *raw, double *sums) {
    using namespace sph;
    if (!d || !exps || !raw || !sums) return SPH_ERR_ARG;
    if (d->n_bins < 1 || d->n_bins > MAX_BINS || d->n_q < 0 || d->n_q > MAXQ || (d->flags & ~ALL_FLAGS)) return SPH_ERR_ARG;
    const int nsum = nsum_of(d);
    finish_all(raw, (int64_t)d->n_bins * nsum, exps, nsum, sums);
    return SPH_OK;
}
