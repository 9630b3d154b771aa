// binned.hip -- weighted sums of any quantities over one or two binned axes (include/summersph.h, sph_binned): the generic
// form of profile.hip.  An axis or a quantity is a context field or a row of the caller's values; the result is, per bin,
// the count, the sum of a weight and the sums of the weight times up to eight quantities (and their squares).
//
// Not part of the step loop: nothing here reads or writes the context's grid, cell table, neighbour list, statistics or
// flags.  The scratch is the one the analysis calls share (analysis_scratch).
//
// Pipeline (all on ctx->stream):
//   binned_keys     every slot -> 64-bit key (bin << 32 | original id), slot; unselected slots get a bin past the last:
//                   n_bins outside the range, n_bins + 1 dropped by SKIP_NAN, n_bins + 2 not owned gas.  The pass reads the
//                   context fields in slot order (coalesced) and the caller's rows through orig[i], and leaves what the sums
//                   need as one record per slot: {w, A_0 .. A_{n_q - 1}}, stride 1 + n_q doubles, staged in LDS so that a
//                   block writes its records as one contiguous run.
//   rocprim radix sort on (bin, id)
//   binned_starts   start[b] = first sorted position of bin b (b in [0, n_bins]; start[n_bins] = the selected count); the
//                   three counts are differences of the starts of the bins past the last: exact, no atomics
//   binned_pieces   the piece shape of reduce_common.hpp, as profile_pieces: one wavefront per piece of PIECE sorted
//                   positions of a bin; a position costs one gather (its record), not one per source
//   binned_final    one wavefront per (bin, sum) adds the bin's pieces
// The reduction shape of a bin depends on its start and length in the sorted (bin, id) sequence alone, and a term w * A
// with w = m is profile.hip's m * q: a ring-binned mass-weighted sum here is bitwise sph_profile's.  No float atomics.
#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <cstring>
#include <vector>

#include "reduce_common.hpp"

// every term in one documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int KB = 256;            // block of every kernel here
constexpr int MAXQ = SPH_BINNED_MAX_Q;
constexpr int ALL_FLAGS = SPH_BINNED_LOG0 | SPH_BINNED_LOG1 | SPH_BINNED_EDGES0 | SPH_BINNED_EDGES1 | SPH_BINNED_SQUARES |
                          SPH_BINNED_SKIP_NAN;

enum { GUESS_LINEAR = 0, GUESS_LOG = 1, SEARCH = 2 };

// a source: a context field in slot order (by_id 0) or a row of the caller's values by original id
struct Axis {
    const double *src;
    const double *edge;            // n + 1 edges (device)
    double lo, scale;              // guess: linear (a - lo) scale, log log(a / lo) scale
    int32_t n, mode, by_id, pad;
};

struct Spec {
    Axis ax[2];
    const double *q[MAXQ];
    const double *m, *rho;         // the weight's fields (slot order); null where the weight does not read them
    uint32_t q_by_id;              // bit k: q[k] is a row
    int32_t n_axes, n_q, weight, skip_nan;
};

// edge[k] <= a < edge[k + 1] against the table; -1 outside [edge[0], edge[n]) (a NaN is outside)
__device__ __forceinline__ int bin_of(const Axis &x, double a) {
    const int n = x.n;
    if (!(a >= x.edge[0] && a < x.edge[n])) return -1;
    int k;
    if (x.mode == SEARCH) {
        int lo = 0, hi = n - 1;                         // the last k with edge[k] <= a
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (x.edge[mid] <= a) lo = mid; else hi = mid - 1;
        }
        k = lo;
    } else {
        // a guess from the spacing, corrected against the table
        const double g = x.mode == GUESS_LOG ? log(a / x.lo) * x.scale : (a - x.lo) * x.scale;
        k = (int)fmin(fmax(floor(g), 0.0), (double)(n - 1));
        while (k > 0 && a < x.edge[k]) k--;
        while (k < n - 1 && a >= x.edge[k + 1]) k++;
    }
    return k;
}

__global__ __launch_bounds__(KB) void binned_keys(const int32_t *__restrict__ orig, int64_t n_slots, int64_t n_owned, Spec s,
                                                  uint32_t n_bins, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                  double *__restrict__ rec) {
    __shared__ double stage[KB * (1 + MAXQ)];
    const int64_t first = (int64_t)blockIdx.x * KB, i = first + threadIdx.x;
    const int stride = 1 + s.n_q;
    double w = 0.0, a[MAXQ];
#pragma unroll
    for (int k = 0; k < MAXQ; k++) a[k] = 0.0;
    if (i < n_slots) {
        const int32_t id = orig[i];
        uint32_t bin = n_bins + 2;                       // not owned gas
        if (id < n_owned) {
            const int k0 = bin_of(s.ax[0], s.ax[0].src[s.ax[0].by_id ? (int64_t)id : i]);
            int k1 = 0;
            if (s.n_axes == 2 && k0 >= 0) k1 = bin_of(s.ax[1], s.ax[1].src[s.ax[1].by_id ? (int64_t)id : i]);
            if (k0 < 0 || k1 < 0) {
                bin = n_bins;                            // outside the range
            } else {
                bool nan = false;
#pragma unroll
                for (int k = 0; k < MAXQ; k++)
                    if (k < s.n_q) {
                        a[k] = s.q[k][(s.q_by_id >> k) & 1u ? (int64_t)id : i];
                        nan = nan || a[k] != a[k];
                    }
                if (s.skip_nan && nan) {
                    bin = n_bins + 1;                    // dropped
                } else {
                    w = 1.0;
                    if (s.weight == SPH_BINNED_W_MASS) w = s.m[i];
                    else if (s.weight == SPH_BINNED_W_VOLUME) w = s.m[i] / s.rho[i];
                    bin = (uint32_t)(k0 * s.ax[1].n + k1);
                }
            }
        }
        keys[i] = ((uint64_t)bin << 32) | (uint64_t)(uint32_t)id;
        vals[i] = (uint32_t)i;
    }
    // the block's records through LDS: its slots are one contiguous run of the record array
    double *r = stage + threadIdx.x * stride;
    r[0] = w;
#pragma unroll
    for (int k = 0; k < MAXQ; k++)
        if (k < s.n_q) r[1 + k] = a[k];
    __syncthreads();
    const int len = (int)min((int64_t)KB, n_slots - first) * stride;
    double *out = rec + first * stride;
    for (int e = threadIdx.x; e < len; e += KB) out[e] = stage[e];
}

// lower bound of (b << 32) in the sorted keys
__device__ __forceinline__ int64_t first_of(const uint64_t *keys, int64_t n, uint64_t b) {
    const uint64_t key = b << 32;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// start[b], b in [0, n_bins]; cnt (may be null): selected = start[n_bins], then the runs of the bins n_bins (outside) and
// n_bins + 1 (dropped)
__global__ __launch_bounds__(KB) void binned_starts(const uint64_t *__restrict__ keys, int64_t n, uint32_t n_bins,
                                                    int32_t *__restrict__ start, int64_t *__restrict__ cnt) {
    const int64_t b = (int64_t)blockIdx.x * KB + threadIdx.x;
    if (b > (int64_t)n_bins) return;
    const int64_t lo = first_of(keys, n, (uint64_t)b);
    start[b] = (int32_t)lo;
    if (b == (int64_t)n_bins && cnt) {
        const int64_t s1 = first_of(keys, n, (uint64_t)n_bins + 1), s2 = first_of(keys, n, (uint64_t)n_bins + 2);
        cnt[0] = lo;
        cnt[1] = s1 - lo;
        cnt[2] = s2 - s1;
    }
}

// one wavefront per piece slot g; gaps (slots no (bin, piece) maps to) return at once.  MQ: the quantities the instance
// has registers for (n_q <= MQ, the tests on k are wave-uniform); SQ: also sum w (A A).
template <int MQ, bool SQ>
__global__ __launch_bounds__(KB) void binned_pieces(const double *__restrict__ rec, int n_q, const uint32_t *__restrict__ vals,
                                                    const int32_t *__restrict__ start, uint32_t n_bins, int64_t n_pieces,
                                                    double *__restrict__ part) {
    const int64_t g = (int64_t)blockIdx.x * (KB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_pieces) return;
    int64_t b, p0, p1;
    if (!piece_locate(start, (int64_t)n_bins, g, b, p0, p1)) return;
    const int stride = 1 + n_q, nsum = 2 + (SQ ? 2 : 1) * n_q;
    double cn = 0.0, cw = 0.0, ca[MQ], cs[MQ];
#pragma unroll
    for (int k = 0; k < MQ; k++) { ca[k] = 0.0; cs[k] = 0.0; }
    for (int64_t p = p0 + lane; p < p1; p += WAVE) {
        const double *r = rec + (int64_t)vals[p] * stride;
        const double w = r[0];
        cn += 1.0;
        cw += w;
#pragma unroll
        for (int k = 0; k < MQ; k++)
            if (k < n_q) {
                const double a = r[1 + k];
                ca[k] += w * a;
                if (SQ) cs[k] += w * (a * a);
            }
    }
    cn = wave_sum(cn);
    cw = wave_sum(cw);
#pragma unroll
    for (int k = 0; k < MQ; k++)
        if (k < n_q) {
            ca[k] = wave_sum(ca[k]);
            if (SQ) cs[k] = wave_sum(cs[k]);
        }
    if (lane == 0) {
        double *o = part + g * nsum;
        o[0] = cn;
        o[1] = cw;
#pragma unroll
        for (int k = 0; k < MQ; k++)
            if (k < n_q) {
                o[2 + k] = ca[k];
                if (SQ) o[2 + n_q + k] = cs[k];
            }
    }
}

// one wavefront per (bin, sum): the bin's pieces in a fixed shape (lane l: pieces l, l + 64, ... in turn, then the butterfly)
__global__ __launch_bounds__(KB) void binned_final(const int32_t *__restrict__ start, uint32_t n_bins, int nsum,
                                                   const double *__restrict__ part, double *__restrict__ sums) {
    const int64_t g = (int64_t)blockIdx.x * (KB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= (int64_t)n_bins * nsum) return;
    const int64_t b = g / nsum;
    const int s = (int)(g - b * nsum);
    const int64_t len = (int64_t)start[b + 1] - start[b];
    const int64_t np = (len + PIECE - 1) / PIECE, base = piece_base(start, b);
    double acc = 0.0;
    for (int64_t k = lane; k < np; k += WAVE) acc += part[(base + k) * nsum + s];
    acc = wave_sum(acc);
    if (lane == 0) sums[g] = acc;
}

template <int MQ>
void launch_pieces(bool sq, unsigned nblk, hipStream_t st, const double *rec, int n_q, const uint32_t *vals,
                   const int32_t *start, uint32_t n_bins, int64_t n_pieces, double *part) {
    if (sq) binned_pieces<MQ, true><<<dim3(nblk), dim3(KB), 0, st>>>(rec, n_q, vals, start, n_bins, n_pieces, part);
    else binned_pieces<MQ, false><<<dim3(nblk), dim3(KB), 0, st>>>(rec, n_q, vals, start, n_bins, n_pieces, part);
}

// the checks that need no context and no table; null: fine
const char *check_desc(const sph_binned_desc *d, const double *edges) {
    for (int k = 0; k < 3; k++)
        if (d->reserved[k] != 0) return "reserved must be 0";
    if (d->flags & ~ALL_FLAGS) return "unknown flags";
    if (d->weight != SPH_BINNED_W_ONE && d->weight != SPH_BINNED_W_MASS && d->weight != SPH_BINNED_W_VOLUME) return "unknown weight";
    if (d->n_axes != 1 && d->n_axes != 2) return "n_axes must be 1 or 2";
    if (d->n[0] < 1 || d->n[1] < 1) return "n[] must be >= 1";
    if (d->n_axes == 1 && d->n[1] != 1) return "n[1] must be 1 with one axis";
    if ((int64_t)d->n[0] * d->n[1] > ((int64_t)1 << 20)) return "n[0] * n[1] must be <= 2^20";
    if (d->n_axes == 1 && (d->flags & (SPH_BINNED_LOG1 | SPH_BINNED_EDGES1))) return "a flag of axis 1 with one axis";
    if (d->n_q < 0 || d->n_q > MAXQ) return "n_q must be 0 .. SPH_BINNED_MAX_Q";
    if (d->n_rows < 0 || d->n_rows > MAX_ROWS) return "n_rows must be 0 .. 16";
    for (int a = 0; a < d->n_axes; a++)
        if (!source_ok(d->axis[a], d->n_rows)) return "an axis source is neither an SPH_F_* id nor a row below n_rows";
    for (int k = 0; k < d->n_q; k++)
        if (!source_ok(d->q[k], d->n_rows)) return "a quantity source is neither an SPH_F_* id nor a row below n_rows";
    bool any_edges = false;
    for (int a = 0; a < d->n_axes; a++) {
        const bool lg = (d->flags & (SPH_BINNED_LOG0 << a)) != 0, ed = (d->flags & (SPH_BINNED_EDGES0 << a)) != 0;
        if (lg && ed) return "LOG and EDGES on the same axis";
        any_edges = any_edges || ed;
        if (ed) continue;
        if (!std::isfinite(d->lo[a]) || !std::isfinite(d->hi[a]) || !(d->lo[a] < d->hi[a])) return "need finite lo < hi";
        if (lg && !(d->lo[a] > 0.0)) return "a logarithmic axis needs lo > 0";
    }
    if (any_edges != (edges != nullptr)) return "edges must be given with SPH_BINNED_EDGES0 / EDGES1 and only then";
    return nullptr;
}

// the caller's table of axis a inside edges: the tables of the axes that have one, in axis order
const double *caller_table(const sph_binned_desc *d, const double *edges, int a) {
    return edges + ((a == 1 && (d->flags & SPH_BINNED_EDGES0)) ? (size_t)d->n[0] + 1 : 0);
}

// edge[k], k in [0, n]: linear lo + (k (hi - lo)) / n, log lo pow(hi / lo, k / n), edge[n] = hi (profile.hip, ring_edges);
// or the caller's table.  null: fine
const char *axis_edges(const sph_binned_desc *d, const double *edges, int a, double *edge) {
    const int n = d->n[a];
    if (d->flags & (SPH_BINNED_EDGES0 << a)) {
        std::memcpy(edge, caller_table(d, edges, a), ((size_t)n + 1) * sizeof(double));
    } else {
        const bool lg = (d->flags & (SPH_BINNED_LOG0 << a)) != 0;
        const double lo = d->lo[a], hi = d->hi[a];
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

}  // namespace

int binned_run(sph_ctx *c, const sph_binned_desc *d, const double *values, const double *edges, double *sums, int64_t n_sums,
               int64_t *counts, bool host) {
    const char *who = "sph_binned";
    if (!d) return arg_error(c, who, "null descriptor");
    if (!sums) return arg_error(c, who, "null output");
    if (const char *why = check_desc(d, edges)) return arg_error(c, who, why);
    const bool squares = (d->flags & SPH_BINNED_SQUARES) != 0;
    const int nq = d->n_q, nsum = 2 + nq * (squares ? 2 : 1), stride = 1 + nq;
    const int64_t n_bins = (int64_t)d->n[0] * d->n[1];
    if (n_sums != n_bins * nsum) return arg_error(c, who, "n_sums != n[0] n[1] (2 + n_q (1 + squares))");
    if ((d->n_rows == 0) != (values == nullptr)) return arg_error(c, who, "values must be given with n_rows > 0 and only then");

    // the edge tables travel in the stream's order from a pinned staging copy (sph_profile's), rewritten only once its
    // last upload is done
    hipStream_t st = c->stream;
    const size_t ne0 = (size_t)d->n[0] + 1, ne = ne0 + (d->n_axes == 2 ? (size_t)d->n[1] + 1 : 0);
    double *edge = nullptr;
    SPH_TRY(table_staging(c, ne, &edge));
    for (int a = 0; a < d->n_axes; a++)
        if (const char *why = axis_edges(d, edges, a, edge + (a ? ne0 : 0))) return arg_error(c, who, why);

    uint32_t rows_used = 0;                              // the rows some source reads
    auto use = [&](int32_t id) {
        if (id < 0) { rows_used |= 1u << (-1 - id); return true; }
        return field_ready(*c, c->variable, id);
    };
    bool fresh = true;
    for (int a = 0; a < d->n_axes; a++) fresh = use(d->axis[a]) && fresh;
    for (int k = 0; k < nq; k++) fresh = use(d->q[k]) && fresh;
    if (d->weight == SPH_BINNED_W_VOLUME) fresh = field_ready(*c, c->variable, SPH_F_RHO) && fresh;
    if (!fresh) {
        c->err = "sph_binned: a field is stale (as sph_download_field would refuse it)";
        return SPH_ERR_STATE;
    }

    const int64_t n = c->n, n_slots = c->cap > 0 ? c->n_slots : 0;
    if (n_slots == 0 || n == 0) {                        // nothing held: zero sums
        SPH_HIP(zero_output(sums, (size_t)n_sums, host, st));
        SPH_HIP(zero_output(counts, 3, host, st));
        return SPH_OK;
    }

    const uint32_t nb = (uint32_t)n_bins;
    const int64_t n_pieces = n_slots / PIECE + n_bins + 1;
    size_t sort_bytes = 0;
    SPH_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)n_slots, 0u, 64u, st));
    uint64_t *keys, *keys_alt;
    uint32_t *vals, *vals_alt;
    char *sort_tmp;
    int32_t *start;
    double *d_edge, *rec, *part, *h_values, *h_sums;
    int64_t *cnt;
    auto layout = [&](Carve cv) {
        keys = cv.take<uint64_t>(n_slots);
        keys_alt = cv.take<uint64_t>(n_slots);
        vals = cv.take<uint32_t>(n_slots);
        vals_alt = cv.take<uint32_t>(n_slots);
        sort_tmp = cv.take<char>(sort_bytes);
        d_edge = cv.take<double>(ne);
        start = cv.take<int32_t>(n_bins + 1);
        rec = cv.take<double>((size_t)stride * (size_t)n_slots);
        part = cv.take<double>((size_t)nsum * (size_t)n_pieces);
        cnt = cv.take<int64_t>(host ? 3 : 0);                                       // the host form's device copy
        h_values = cv.take<double>(host ? (size_t)d->n_rows * (size_t)n : 0);      // the host form's device copies
        h_sums = cv.take<double>(host ? n_sums : 0);
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    double *d_out = host ? h_sums : sums;
    const double *d_values = host ? h_values : values;
    if (host) {
        SPH_TRY(analysis_pinned(c));
        SPH_HIP(upload_rows(h_values, values, d->n_rows, rows_used, (size_t)n, st));
    }
    SPH_HIP(hipMemcpyAsync(d_edge, edge, ne * sizeof(double), hipMemcpyHostToDevice, st));
    SPH_HIP(hipEventRecord(c->prf_evt, st));

    auto source = [&](int32_t id) { return id >= 0 ? c->f[id] : d_values + (size_t)(-1 - id) * (size_t)n; };
    Spec s{};
    for (int a = 0; a < 2; a++) {
        Axis &x = s.ax[a];
        x.n = 1;
        if (a >= d->n_axes) continue;
        x.src = source(d->axis[a]);
        x.by_id = d->axis[a] < 0;
        x.edge = d_edge + (a ? ne0 : 0);
        x.n = d->n[a];
        x.lo = d->lo[a];
        if (d->flags & (SPH_BINNED_EDGES0 << a)) {
            x.mode = SEARCH;
        } else if (d->flags & (SPH_BINNED_LOG0 << a)) {
            x.mode = GUESS_LOG;
            x.scale = (double)x.n / std::log(d->hi[a] / d->lo[a]);
        } else {
            x.mode = GUESS_LINEAR;
            x.scale = (double)x.n / (d->hi[a] - d->lo[a]);
        }
    }
    for (int k = 0; k < nq; k++) {
        s.q[k] = source(d->q[k]);
        if (d->q[k] < 0) s.q_by_id |= 1u << k;
    }
    s.m = d->weight != SPH_BINNED_W_ONE ? c->f[SPH_F_M] : nullptr;
    s.rho = d->weight == SPH_BINNED_W_VOLUME ? c->f[SPH_F_RHO] : nullptr;
    s.n_axes = d->n_axes;
    s.n_q = nq;
    s.weight = d->weight;
    s.skip_nan = (d->flags & SPH_BINNED_SKIP_NAN) != 0;

    int64_t *d_cnt = host ? cnt : counts;                // device form: straight into the caller's (or nowhere)
    binned_keys<<<dim3(blocks(n_slots, KB)), dim3(KB), 0, st>>>(c->orig, n_slots, c->n_owned, s, nb, keys, vals, rec);
    SPH_HIP(hipGetLastError());
    unsigned bbits = 1;
    while (bbits < 32 && ((uint64_t)1 << bbits) <= (uint64_t)nb + 2) bbits++;       // the bins past the last: n_bins .. n_bins + 2
    size_t tmp = sort_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, keys, keys_alt, vals, vals_alt, (size_t)n_slots, 0u, 32u + bbits, st));
    binned_starts<<<dim3(blocks(n_bins + 1, KB)), dim3(KB), 0, st>>>(keys_alt, n_slots, nb, start, d_cnt);
    const int wpb = KB / WAVE;
    const unsigned pblk = blocks(n_pieces, wpb);
    if (nq <= 1) launch_pieces<1>(squares, pblk, st, rec, nq, vals_alt, start, nb, n_pieces, part);
    else if (nq <= 4) launch_pieces<4>(squares, pblk, st, rec, nq, vals_alt, start, nb, n_pieces, part);
    else launch_pieces<MAXQ>(squares, pblk, st, rec, nq, vals_alt, start, nb, n_pieces, part);
    binned_final<<<dim3(blocks(n_bins * nsum, wpb)), dim3(KB), 0, st>>>(start, nb, nsum, part, d_out);
    SPH_HIP(hipGetLastError());
    if (!host) return SPH_OK;
    // host form: the sums and the counts in one read-back
    SPH_HIP(hipMemcpyAsync(c->rnd_pinned, cnt, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipMemcpyAsync(sums, d_out, (size_t)n_sums * sizeof(double), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    if (counts) std::memcpy(counts, c->rnd_pinned, 3 * sizeof(int64_t));
    return SPH_OK;
}

}  // namespace sph

extern "C" int sph_binned_edges(const sph_binned_desc *d, const double *edges, int32_t axis, double *out) {
    using namespace sph;
    if (!d || !out) return SPH_ERR_ARG;
    if (check_desc(d, edges)) return SPH_ERR_ARG;
    if (axis < 0 || axis >= d->n_axes) return SPH_ERR_ARG;
    // every table of the call must stand, not only the one asked for
    std::vector<double> other;
    for (int a = 0; a < d->n_axes; a++) {
        double *t = out;
        if (a != axis) { other.resize((size_t)d->n[a] + 1); t = other.data(); }
        if (axis_edges(d, edges, a, t)) return SPH_ERR_ARG;
    }
    return SPH_OK;
}
