// peaks.hip -- density-peak clumps of the owned gas: every particle climbs to its densest neighbour, each basin is a clump,
// and basins merge across saddles that are high compared with the lower peak (include/summersph.h, sph_peaks).
//
// Not part of the step loop: nothing here reads or writes the context's grid, cell table, neighbour list, statistics or
// flags.  The scratch is the one the analysis calls share (analysis_scratch).
//
// Pipeline (all on ctx->stream):
//   groups_front     (groups.hip) selection, box, cell keys, sort, {x, y, z, h} records and the hashed cell table;
//                    parent[id] = id for every selected owned id, -1 for every other
//   peaks_gather     sorted position p: rho in sorted order
//   peaks_hop        one lane per sorted position over the full 27-cell stencil: the highest (rho, then the smaller id) of
//                    the particle and its neighbours, kept in registers -> parent[id] = next.  No atomics.
//   peaks_jump       rounds of pointer jumping in separate launches, JUMP links per round: parent[id] = peak
//   peaks_edges<0>   half stencil (every pair once, as groups_link): neighbour pairs whose peaks differ, counted per lane
//   rocprim exclusive scan -> every lane's offset and the total T
//   peaks_flags / rocprim exclusive scan / peaks_compact: the P raw peaks in id order, their ids and rho.  T and P are
//                    read back (first wait); the pair buffers are sized from T: where the scratch is too small it grows
//                    and the pipeline starts again
//   peaks_edges<1>   the same walk: (min peak << 32 | max peak, ordered bits of min(rho_i, rho_j)) per pair
//   rocprim radix sort by key, reduce_by_key with an integer maximum -> the distinct edges and S, their count E read
//                    back (second wait)
//   peaks_edge_keys / rocprim radix sort (stable): the edges by S descending, key ascending
//   peaks_edge_idx   both ends of every edge as positions among the raw peaks -> edges, S and the peaks' rho to the host
//                    (third wait: 16 bytes per edge, 8 per peak)
//   host             the merge of summersph.h as a union-find over the E edges and P peaks; the top of every peak and
//                    S_out of every top go back up (12 bytes per peak)
//   peaks_scatter    top[peak], sout[top] from the uploaded lists
//   peaks_assign     every owned id: parent[id] = the top of its peak's component, or -1 when that top is below peak_min;
//                    raw peaks counted per top and in all (integer atomics)
//   peaks_minid      atomicMin: the smallest member id of every top
//   peaks_root       parent[id] = that smallest id (a root is its own parent, as groups_tail wants); rtop[root] = top
//   groups_tail      (groups.hip) count, numbering, member sort, labels, the two reductions -> a 21-column table
//   peaks_table      widens the rows to 23 columns (S_out, raw peaks) and writes the counts
//
// Stale loads.  peaks_hop stores parent[] of its own id only and reads none.  peaks_jump follows parent links with plain
// loads while other lanes shorten them: every value parent[x] ever holds is a node of x's ascending chain that is not
// below an earlier value, so a stale load returns an older node of the same chain, the walk still ends at the chain's
// peak or at a node nearer to it, and 16^rounds >= n links are spanned whatever the schedule.  The peak of every particle,
// and with it every edge, S (an integer maximum), label and table entry, is independent of the schedule.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cell_table.hpp"

#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int PB = 256;                    // block of every kernel here
constexpr int JUMP = 16;                   // links a lane follows per jump round

// on the device: distinct edges
struct PInfo { unsigned long long n_edges; };

// a double as an unsigned integer of the same order (any sign; -0 below +0), and back
__device__ __host__ __forceinline__ uint64_t ordered_bits(double v) {
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
inline double from_ordered_bits(uint64_t u) {
    u = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
    double v;
    memcpy(&v, &u, sizeof v);
    return v;
}

__global__ __launch_bounds__(PB) void peaks_gather(const double *__restrict__ rho, const uint32_t *__restrict__ sval,
                                                   const GroupsInfo *__restrict__ info, int64_t n_slots,
                                                   double *__restrict__ srho) {
    const int64_t p = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (p >= n_slots || p >= info->n_sel) return;
    srho[p] = rho[sval[p]];
}

__device__ __forceinline__ bool cell_of(const int64_t c[3], int o, uint64_t &nk) {
    const int64_t n0 = c[0] + o / 9 - 1, n1 = c[1] + (o / 3) % 3 - 1, n2 = c[2] + o % 3 - 1;
    if (n0 < 0 || n1 < 0 || n2 < 0 || n0 > (int64_t)AXIS_MASK || n1 > (int64_t)AXIS_MASK || n2 > (int64_t)AXIS_MASK) return false;
    nk = ((uint64_t)n0 << (2 * AXIS_BITS)) | ((uint64_t)n1 << AXIS_BITS) | (uint64_t)n2;
    return true;
}

__device__ __forceinline__ bool neighbours(const double4 &r, const double4 &s, double link, double b2, int32_t link_h) {
    const double dx = r.x - s.x, dy = r.y - s.y, dz = r.z - s.z;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    double bb = b2;
    if (link_h) {
        const double b = link * fmax(r.w, s.w);
        bb = b * b;
    }
    return d2 < bb;
}

// next[id] = the highest of the particle and its neighbours (rho, then the smaller original id)
__global__ __launch_bounds__(PB) void peaks_hop(const double4 *__restrict__ rec, const int32_t *__restrict__ sid,
                                                const double *__restrict__ srho, const uint64_t *__restrict__ skey,
                                                const GroupsInfo *__restrict__ info, int64_t n_slots,
                                                const Ent *__restrict__ tab, uint64_t mask, double link, double b2,
                                                int32_t link_h, int64_t n_owned, int32_t *__restrict__ parent) {
    const int64_t p = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (p >= n_slots || p >= info->n_sel) return;
    const double4 r = rec[p];
    const uint64_t key = skey[p];
    const int64_t c[3] = {(int64_t)(key >> (2 * AXIS_BITS)), (int64_t)((key >> AXIS_BITS) & AXIS_MASK), (int64_t)(key & AXIS_MASK)};
    const int32_t me = sid[p];
    double best_rho = srho[p];
    int32_t best_id = me;
    for (int o = 0; o < 27; o++) {
        uint64_t nk;
        if (!cell_of(c, o, nk)) continue;
        const int64_t t = hash_slot(tab, mask, nk);
        if (t < 0) continue;
        const int64_t q1 = tab[t].end;
        for (int64_t q = tab[t].start; q < q1; q++) {
            if (q == p || !neighbours(r, rec[q], link, b2, link_h)) continue;
            const double rq = srho[q];
            const int32_t iq = sid[q];
            if (rq > best_rho || (rq == best_rho && iq < best_id)) { best_rho = rq; best_id = iq; }
        }
    }
    if (me >= 0 && me < n_owned) parent[me] = best_id;
}

// one round of pointer jumping: parent[x] = the node JUMP links up (or the peak).  Rounds are separate launches.
__global__ __launch_bounds__(PB) void peaks_jump(int32_t *parent, int64_t n_owned) {
    const int64_t x = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (x >= n_owned) return;
    const int32_t p0 = parent[x];
    if (p0 < 0 || p0 == x) return;
    int32_t p = p0;
    for (int k = 0; k < JUMP; k++) {
        const int32_t q = parent[p];
        if (q == p) break;
        p = q;
    }
    if (p != p0) parent[x] = p;
}

// the neighbour pairs (q > p in sorted order) whose peaks differ.  EMIT 0: their number per lane; EMIT 1: key and saddle
// value of each, from the lane's offset on (the two walks enumerate the same pairs in the same order)
template <int EMIT>
__global__ __launch_bounds__(PB) void peaks_edges(const double4 *__restrict__ rec, const int32_t *__restrict__ sid,
                                                  const double *__restrict__ srho, const uint64_t *__restrict__ skey,
                                                  const GroupsInfo *__restrict__ info, int64_t n_slots,
                                                  const Ent *__restrict__ tab, uint64_t mask, double link, double b2,
                                                  int32_t link_h, const int32_t *__restrict__ parent,
                                                  uint32_t *__restrict__ count, const uint64_t *__restrict__ offset,
                                                  int64_t cap, uint64_t *__restrict__ ekey, uint64_t *__restrict__ eval) {
    const int64_t p = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (p > n_slots) return;
    if (p == n_slots || p >= info->n_sel) {                     // count[n_slots] closes the scan: offset[n_slots] = T
        if (!EMIT) count[p] = 0;
        return;
    }
    const double4 r = rec[p];
    const uint64_t key = skey[p];
    const int64_t c[3] = {(int64_t)(key >> (2 * AXIS_BITS)), (int64_t)((key >> AXIS_BITS) & AXIS_MASK), (int64_t)(key & AXIS_MASK)};
    const int32_t pk = parent[sid[p]];
    const double rp = srho[p];
    uint32_t found = 0;
    int64_t at = EMIT ? (int64_t)offset[p] : 0;
    for (int o = 13; o < 27; o++) {
        uint64_t nk;
        if (!cell_of(c, o, nk)) continue;
        const int64_t t = hash_slot(tab, mask, nk);
        if (t < 0) continue;
        const int64_t q0 = o == 13 ? p + 1 : tab[t].start, q1 = tab[t].end;
        for (int64_t q = q0; q < q1; q++) {
            if (!neighbours(r, rec[q], link, b2, link_h)) continue;
            const int32_t qk = parent[sid[q]];
            if (qk == pk) continue;
            if (EMIT) {
                if (at < cap) {
                    const uint32_t a = (uint32_t)min(pk, qk), b = (uint32_t)max(pk, qk);
                    ekey[at] = ((uint64_t)a << 32) | (uint64_t)b;
                    eval[at] = ordered_bits(fmin(rp, srho[q]));
                }
                at++;
            } else {
                found++;
            }
        }
    }
    if (!EMIT) count[p] = found;
}

// sort keys of the second sort: S descending = the complement ascending
__global__ __launch_bounds__(PB) void peaks_edge_keys(const uint64_t *__restrict__ s, int64_t n_edges, uint64_t *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (e < n_edges) out[e] = ~s[e];
}

__global__ __launch_bounds__(PB) void peaks_edge_idx(const uint64_t *__restrict__ ekey, int64_t n_edges, int64_t n_owned,
                                                     const uint32_t *__restrict__ pidx, int32_t *__restrict__ ea,
                                                     int32_t *__restrict__ eb) {
    const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (e >= n_edges) return;
    const int64_t a = (int64_t)(ekey[e] >> 32), b = (int64_t)(ekey[e] & 0xffffffffull);
    ea[e] = a < n_owned ? (int32_t)pidx[a] : 0;
    eb[e] = b < n_owned ? (int32_t)pidx[b] : 0;
}

// flag[x] = 1 for a raw peak (flag[n_owned] = 0 closes the scan: pidx[n_owned] = the raw peaks)
__global__ __launch_bounds__(PB) void peaks_flags(const int32_t *__restrict__ parent, int64_t n_owned,
                                                  const GroupsInfo *__restrict__ info, uint32_t *__restrict__ flag) {
    const int64_t x = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (x > n_owned) return;
    flag[x] = (x < n_owned && info->n_groups >= 0 && parent[x] == (int32_t)x) ? 1u : 0u;
}

// the raw peaks in id order: their ids and rho (the host's merge works on these positions)
__global__ __launch_bounds__(PB) void peaks_compact(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pidx,
                                                    int64_t n_owned, const double *__restrict__ rho,
                                                    const int32_t *__restrict__ inv_slot, int32_t *__restrict__ plist,
                                                    double *__restrict__ prho) {
    const int64_t x = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (x >= n_owned || !flag[x]) return;
    const uint32_t k = pidx[x];
    if ((int64_t)k >= n_owned) return;
    plist[k] = (int32_t)x;
    prho[k] = rho[inv_slot[x]];
}

// slot of every owned id (the context's own inverse may be stale between a ghost swap and the next build)
__global__ __launch_bounds__(PB) void peaks_slots(const int32_t *__restrict__ orig, int64_t n_slots, int64_t n_owned,
                                                  int32_t *__restrict__ inv_slot) {
    const int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (i >= n_slots) return;
    const int32_t id = orig[i];
    if (id >= 0 && id < n_owned) inv_slot[id] = (int32_t)i;
}

__global__ __launch_bounds__(PB) void peaks_scatter(const int32_t *__restrict__ plist, const int32_t *__restrict__ tops,
                                                    const double *__restrict__ souts, int64_t n_peaks, int64_t n_owned,
                                                    int32_t *__restrict__ top, double *__restrict__ sout) {
    const int64_t k = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (k >= n_peaks) return;
    const int32_t id = plist[k], tk = tops[k];
    if (id < 0 || id >= n_owned || tk < 0 || tk >= n_peaks) return;
    top[id] = plist[tk];
    sout[id] = souts[k];
}

// parent[id]: peak -> the top of the peak's component, or -1 when the top is below peak_min; raw peaks per top
__global__ __launch_bounds__(PB) void peaks_assign(int32_t *__restrict__ parent, const int32_t *__restrict__ top,
                                                   const double *__restrict__ rho, const int32_t *__restrict__ inv_slot,
                                                   int64_t n_owned, double peak_min, const GroupsInfo *__restrict__ info,
                                                   int32_t *__restrict__ npk) {
    const int64_t x = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (x >= n_owned || info->n_groups < 0) return;
    const int32_t pk = parent[x];
    if (pk < 0) return;
    const int32_t t0 = top[pk];
    const int32_t t = t0 >= 0 ? t0 : pk;
    if (pk == (int32_t)x) atomicAdd(&npk[t], 1);
    parent[x] = rho[inv_slot[t]] < peak_min ? -1 : t;
}

__global__ __launch_bounds__(PB) void peaks_minid(const int32_t *__restrict__ parent, int64_t n_owned, int32_t *__restrict__ minid) {
    const int64_t x = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (x >= n_owned) return;
    const int32_t t = parent[x];
    if (t >= 0) atomicMin(&minid[t], (int32_t)x);
}

__global__ __launch_bounds__(PB) void peaks_root(int32_t *__restrict__ parent, const int32_t *__restrict__ minid, int64_t n_owned,
                                                 int32_t *__restrict__ rtop) {
    const int64_t x = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (x >= n_owned) return;
    const int32_t t = parent[x];
    if (t < 0) return;
    const int32_t r = minid[t];
    if (t == (int32_t)x) rtop[r] = t;
    parent[x] = r;
}

// rows of 21 columns -> rows of 23 (S_out and the raw peaks of the component's top); the counts
__global__ __launch_bounds__(PB) void peaks_table(const double *__restrict__ t21, int64_t rows, const GroupsInfo *__restrict__ info,
                                                  const PInfo *__restrict__ pinfo, const uint32_t *__restrict__ n_peaks,
                                                  const int32_t *__restrict__ rtop,
                                                  const double *__restrict__ sout, const int32_t *__restrict__ npk,
                                                  int64_t n_owned, double *__restrict__ table, int64_t *__restrict__ counts) {
    const int64_t g = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (g == 0) {
        counts[0] = info->n_groups;
        counts[1] = (int64_t)*n_peaks;
        counts[2] = (int64_t)pinfo->n_edges;
    }
    if (g >= rows || g >= info->n_groups) return;
    const double *s = t21 + g * SPH_GROUPS_NCOL;
    double *t = table + g * SPH_PEAKS_NCOL;
    for (int k = 0; k < SPH_GROUPS_NCOL; k++) t[k] = s[k];
    const int64_t r = (int64_t)s[20];
    const int32_t top = (r >= 0 && r < n_owned) ? rtop[r] : -1;
    t[21] = top >= 0 ? sout[top] : 0.0;
    t[22] = top >= 0 ? (double)npk[top] : 0.0;
}

// the merge of summersph.h over the sorted edges.  Peaks are named by their position in id order (so the smaller
// position is the smaller id): tops[k] = the top of peak k's component, souts[k] = S_out where k is a top
void merge_edges(const std::vector<int32_t> &ea, const std::vector<int32_t> &eb, const std::vector<uint64_t> &eneg,
                 const std::vector<double> &prho, double contrast, std::vector<int32_t> &tops, std::vector<double> &souts) {
    const size_t E = ea.size(), P = prho.size();
    std::vector<int32_t> comp(P), ctop(P);          // union-find parent and, for a root, its top
    for (size_t k = 0; k < P; k++) comp[k] = ctop[k] = (int32_t)k;
    auto find = [&](int32_t k) {
        while (comp[k] != k) { comp[k] = comp[comp[k]]; k = comp[k]; }
        return k;
    };
    auto above = [&](int32_t a, int32_t b) { return prho[a] > prho[b] || (prho[a] == prho[b] && a < b); };
    for (size_t e = 0; e < E; e++) {
        int32_t A = find(ea[e]), B = find(eb[e]);
        if (A == B) continue;
        if (!above(ctop[A], ctop[B])) std::swap(A, B);
        const double S = from_ordered_bits(~eneg[e]);
        const double lim = contrast * S;
        if (prho[ctop[B]] < lim) comp[B] = A;        // A keeps its top, which is above B's
    }
    tops.resize(P);
    souts.assign(P, 0.0);
    for (size_t k = 0; k < P; k++) tops[k] = ctop[find((int32_t)k)];
    for (size_t e = 0; e < E; e++) {
        const int32_t A = tops[ea[e]], B = tops[eb[e]];
        if (A == B) continue;
        const double S = from_ordered_bits(~eneg[e]);
        souts[A] = std::max(souts[A], S);
        souts[B] = std::max(souts[B], S);
    }
}

}  // namespace

int peaks_run(sph_ctx *c, const sph_peaks_desc *d, int32_t *labels, int64_t n_labels, double *table, int64_t max_groups,
              int64_t *counts, bool host) {
    const char *who = "sph_peaks";
    if (!d) return arg_error(c, who, "null descriptor");
    if (!counts) return arg_error(c, who, "null counts pointer");
    if (d->reserved != 0) return arg_error(c, who, "reserved must be 0");
    if (d->flags & ~SPH_PEAKS_LINK_H) return arg_error(c, who, "unknown flags");
    if (!(d->link > 0.0) || !std::isfinite(d->link)) return arg_error(c, who, "link must be finite and > 0");
    if (std::isnan(d->rho_min)) return arg_error(c, who, "rho_min is NaN");
    if (std::isnan(d->peak_min)) return arg_error(c, who, "peak_min is NaN");
    if (!(d->contrast >= 1.0)) return arg_error(c, who, "contrast must be >= 1");
    for (int a = 0; a < 3; a++)
        if (std::isnan(d->clip_lo[a]) || std::isnan(d->clip_hi[a])) return arg_error(c, who, "the clip box has a NaN");
    if (d->min_members < 1) return arg_error(c, who, "min_members must be >= 1");
    if (labels && n_labels != c->n) return arg_error(c, who, "n_labels != sph_count");
    if (max_groups < 0) return arg_error(c, who, "max_groups < 0");
    if (table && max_groups == 0) return arg_error(c, who, "a table needs max_groups > 0");
    if (!field_ready(*c, c->variable, SPH_F_RHO)) { c->err = "sph_peaks: rho is stale (call sph_density)"; return SPH_ERR_STATE; }
    const bool link_h = (d->flags & SPH_PEAKS_LINK_H) != 0;
    if (link_h && !c->variable && !(c->p.h > 0.0 && std::isfinite(c->p.h))) {
        c->err = "sph_peaks: SPH_PEAKS_LINK_H needs h > 0";
        return SPH_ERR_STATE;
    }

    hipStream_t st = c->stream;
    const int64_t n = c->n, no = c->n_owned;
    const int64_t ns = c->cap > 0 ? c->n_slots : 0;
    if (!table) max_groups = 0;
    if (ns == 0 || no == 0) {                       // nothing owned: no group, every label -1
        if (host) {
            if (labels) std::fill(labels, labels + n, -1);
            std::fill(counts, counts + SPH_PEAKS_NCOUNT, (int64_t)0);
        } else {
            if (labels && n > 0) SPH_HIP(hipMemsetAsync(labels, 0xff, (size_t)n * sizeof(int32_t), st));
            SPH_HIP(hipMemsetAsync(counts, 0, SPH_PEAKS_NCOUNT * sizeof(int64_t), st));
        }
        return SPH_OK;
    }
    GroupsWork w{};
    groups_sizes(c, d->min_members, max_groups, w);
    const int64_t rows = w.rows;
    SPH_TRY(analysis_pinned(c));

    GroupsSel s{};
    s.rho_min = d->rho_min;
    s.rho_cap = 1.7976931348623157e308;              // a non-finite rho is never selected
    for (int a = 0; a < 3; a++) { s.clip_lo[a] = d->clip_lo[a]; s.clip_hi[a] = d->clip_hi[a]; }
    s.link = d->link;
    s.fixed_h = c->p.h;
    s.hf = c->variable ? c->f[SPH_F_H] : nullptr;
    s.link_h = link_h ? 1 : 0;
    const double b2 = d->link * d->link;
    const double *rho = c->f[SPH_F_RHO];
    const uint64_t mask = (uint64_t)(w.tl - 1);

    double *srho, *sout, *t21, *prho, *up_sout, *h_table;
    int32_t *inv_slot, *top, *npk, *minid, *rtop, *plist, *up_tops, *h_labels;
    uint32_t *pcount, *flag, *pidx;
    uint64_t *poff, *ekey, *ekey_alt, *eval, *eval_alt;
    char *etmp;
    PInfo *pinfo;
    int64_t *d_counts_own;
    size_t etmp_bytes = 0;
    int64_t cap = 0;                                 // pairs the edge buffers hold
    auto layout = [&](Carve cv) {
        groups_take(w, cv);
        srho = cv.take<double>(ns);
        inv_slot = cv.take<int32_t>(no);
        top = cv.take<int32_t>(no);
        npk = cv.take<int32_t>(no);
        minid = cv.take<int32_t>(no);
        rtop = cv.take<int32_t>(no);
        sout = cv.take<double>(no);
        flag = cv.take<uint32_t>(no + 1);
        pidx = cv.take<uint32_t>(no + 1);
        plist = cv.take<int32_t>(no);
        prho = cv.take<double>(no);
        up_tops = cv.take<int32_t>(no);
        up_sout = cv.take<double>(no);
        pcount = cv.take<uint32_t>(ns + 1);
        poff = cv.take<uint64_t>(ns + 1);
        pinfo = cv.take<PInfo>(1);
        d_counts_own = cv.take<int64_t>(SPH_PEAKS_NCOUNT);
        t21 = cv.take<double>(SPH_GROUPS_NCOL * (size_t)rows);
        h_labels = cv.take<int32_t>(host && labels ? n : 0);                     // the host form's device copies
        h_table = cv.take<double>(host ? SPH_PEAKS_NCOL * (size_t)rows : 0);
        ekey = cv.take<uint64_t>(cap);
        ekey_alt = cv.take<uint64_t>(cap);
        eval = cv.take<uint64_t>(cap);
        eval_alt = cv.take<uint64_t>(cap);
        etmp = cv.take<char>(etmp_bytes);
        return cv.bytes;
    };
    auto edge_tmp = [&](int64_t pairs) {             // temporary storage of the scan, the two sorts and the reduction
        size_t a = 0, b = 0, e = 0, f = 0;
        (void)rocprim::exclusive_scan(nullptr, f, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)(no + 1),
                                      rocprim::plus<uint32_t>(), st);
        (void)rocprim::exclusive_scan(nullptr, a, (uint32_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, (size_t)(ns + 1),
                                      rocprim::plus<uint64_t>(), st);
        if (pairs > 0) {
            (void)rocprim::radix_sort_pairs(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr,
                                            (uint64_t *)nullptr, (size_t)pairs, 0u, 64u, st);
            (void)rocprim::reduce_by_key(nullptr, e, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)pairs, (uint64_t *)nullptr,
                                         (uint64_t *)nullptr, (unsigned long long *)nullptr, rocprim::maximum<uint64_t>(),
                                         rocprim::equal_to<uint64_t>(), st);
        }
        return std::max(std::max(a, f), std::max(b, e));
    };
    // the edge buffers take what the scratch already has room for (a bisection over the layout), at least four pairs per
    // slot: a call on a set like the last one then fits at once
    auto fits = [&](int64_t pairs) {
        cap = pairs;
        etmp_bytes = edge_tmp(cap);
        return layout(Carve{}) <= c->rnd_bytes;
    };
    int64_t cap_lo = 4 * ns;
    if (fits(cap_lo)) {
        int64_t cap_hi = cap_lo + (int64_t)(c->rnd_bytes / 64) + 1;              // 64 bytes per pair: cannot fit
        while (cap_hi - cap_lo > 1) {
            const int64_t mid = cap_lo + (cap_hi - cap_lo) / 2;
            if (fits(mid)) cap_lo = mid; else cap_hi = mid;
        }
    }
    fits(cap_lo);
    int rounds = 1;
    for (double span = JUMP; span < (double)no; span *= JUMP) rounds++;
    char *buf = nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); };
    double at_pairs = 0.0, at_edges = 0.0, at_list = 0.0, at_merged = 0.0;      // SPH_PEAKS_TIMING: ms since the start
    int64_t T = 0, P = 0;                            // pairs that cross basins, raw peaks
    int passes = 0;
    for (int attempt = 0;; attempt++) {
        passes++;
        SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
        layout(Carve{buf});
        SPH_TRY(groups_front(c, s, w));
        SPH_HIP(hipMemsetAsync(inv_slot, 0, (size_t)no * sizeof(int32_t), st));
        peaks_gather<<<dim3(blocks(ns, PB)), dim3(PB), 0, st>>>(rho, w.vals_alt, w.info, ns, srho);
        peaks_slots<<<dim3(blocks(ns, PB)), dim3(PB), 0, st>>>(c->orig, ns, no, inv_slot);
        peaks_hop<<<dim3(blocks(ns, PB)), dim3(PB), 0, st>>>(w.rec, w.sid, srho, w.keys_alt, w.info, ns, w.tab, mask, d->link, b2,
                                                              s.link_h, no, w.parent);
        SPH_HIP(hipGetLastError());
        for (int r = 0; r < rounds; r++) peaks_jump<<<dim3(blocks(no, PB)), dim3(PB), 0, st>>>(w.parent, no);
        peaks_edges<0><<<dim3(blocks(ns + 1, PB)), dim3(PB), 0, st>>>(w.rec, w.sid, srho, w.keys_alt, w.info, ns, w.tab, mask, d->link,
                                                                      b2, s.link_h, w.parent, pcount, nullptr, 0, nullptr, nullptr);
        SPH_HIP(hipGetLastError());
        size_t tmp = etmp_bytes;
        SPH_HIP(rocprim::exclusive_scan(etmp, tmp, pcount, poff, (uint64_t)0, (size_t)(ns + 1), rocprim::plus<uint64_t>(), st));
        SPH_HIP(hipMemcpyAsync(c->rnd_pinned, poff + ns, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        // the raw peaks in id order (their count comes back with T)
        peaks_flags<<<dim3(blocks(no + 1, PB)), dim3(PB), 0, st>>>(w.parent, no, w.info, flag);
        tmp = etmp_bytes;
        SPH_HIP(rocprim::exclusive_scan(etmp, tmp, flag, pidx, 0u, (size_t)(no + 1), rocprim::plus<uint32_t>(), st));
        peaks_compact<<<dim3(blocks(no, PB)), dim3(PB), 0, st>>>(flag, pidx, no, rho, inv_slot, plist, prho);
        SPH_HIP(hipGetLastError());
        SPH_HIP(hipMemcpyAsync(c->rnd_pinned + 1, pidx + no, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));                            // first wait: the pairs that cross basins, the peaks
        std::memcpy(&T, c->rnd_pinned, sizeof(int64_t));
        uint32_t p32 = 0;
        std::memcpy(&p32, c->rnd_pinned + 1, sizeof(uint32_t));
        P = (int64_t)p32;
        at_pairs = since();
        if (T <= cap) break;
        if (attempt > 0) { c->err = "sph_peaks: the pair count changed between two passes"; return SPH_ERR_STATE; }
        cap = T;                                                       // the scratch grows: its contents go, so start again
        etmp_bytes = edge_tmp(cap);
    }
    // distinct edges with S, sorted by (S descending, key ascending)
    int64_t E = 0;
    SPH_HIP(hipMemsetAsync(pinfo, 0, sizeof(PInfo), st));
    if (T > 0) {
        peaks_edges<1><<<dim3(blocks(ns + 1, PB)), dim3(PB), 0, st>>>(w.rec, w.sid, srho, w.keys_alt, w.info, ns, w.tab, mask, d->link,
                                                                      b2, s.link_h, w.parent, nullptr, poff, cap, ekey, eval);
        SPH_HIP(hipGetLastError());
        size_t tmp = etmp_bytes;
        SPH_HIP(rocprim::radix_sort_pairs(etmp, tmp, ekey, ekey_alt, eval, eval_alt, (size_t)T, 0u, 64u, st));
        tmp = etmp_bytes;
        SPH_HIP(rocprim::reduce_by_key(etmp, tmp, ekey_alt, eval_alt, (size_t)T, ekey, eval, &pinfo->n_edges,
                                       rocprim::maximum<uint64_t>(), rocprim::equal_to<uint64_t>(), st));
        SPH_HIP(hipMemcpyAsync(c->rnd_pinned, &pinfo->n_edges, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));                            // second wait: the distinct edges
        std::memcpy(&E, c->rnd_pinned, sizeof(int64_t));
        at_edges = since();
        if (E < 0 || E > T) { c->err = "sph_peaks: bad edge count"; return SPH_ERR_STATE; }
    }
    double merge_ms = 0.0;
    std::vector<int32_t> m_tops;
    std::vector<double> m_sout;
    if (P > no) { c->err = "sph_peaks: bad peak count"; return SPH_ERR_STATE; }
    if (E > 0) {
        // keys (complement of S) from eval into eval_alt; sorted: the complements in eval, the edge keys in ekey_alt
        peaks_edge_keys<<<dim3(blocks(E, PB)), dim3(PB), 0, st>>>(eval, E, eval_alt);
        size_t tmp = etmp_bytes;
        SPH_HIP(rocprim::radix_sort_pairs(etmp, tmp, eval_alt, eval, ekey, ekey_alt, (size_t)E, 0u, 64u, st));
        int32_t *ea = reinterpret_cast<int32_t *>(eval_alt), *eb = ea + E;       // 8 E bytes of the 8 cap
        peaks_edge_idx<<<dim3(blocks(E, PB)), dim3(PB), 0, st>>>(ekey_alt, E, no, pidx, ea, eb);
        SPH_HIP(hipGetLastError());
        std::vector<int32_t> ha((size_t)E), hb((size_t)E);
        std::vector<uint64_t> hs((size_t)E);
        std::vector<double> hr((size_t)P);
        SPH_HIP(hipMemcpyAsync(ha.data(), ea, (size_t)E * 4, hipMemcpyDeviceToHost, st));
        SPH_HIP(hipMemcpyAsync(hb.data(), eb, (size_t)E * 4, hipMemcpyDeviceToHost, st));
        SPH_HIP(hipMemcpyAsync(hs.data(), eval, (size_t)E * 8, hipMemcpyDeviceToHost, st));
        SPH_HIP(hipMemcpyAsync(hr.data(), prho, (size_t)P * 8, hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));                            // third wait: the edge list, the peaks' rho
        at_list = since();
        for (int64_t e = 0; e < E; e++)
            if (ha[e] < 0 || ha[e] >= P || hb[e] < 0 || hb[e] >= P) { c->err = "sph_peaks: bad edge"; return SPH_ERR_STATE; }
        const auto m0 = std::chrono::steady_clock::now();
        merge_edges(ha, hb, hs, hr, d->contrast, m_tops, m_sout);
        merge_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - m0).count();
        at_merged = since();
    }
    // SPH_PEAKS_TIMING: one line per call for profiles/peaks_time.py (pairs, edges, passes over the pairs, the host merge,
    // and when the three waits and the merge ended, in ms since the call began)
    if (switches().peaks_timing)
        fprintf(stderr, "sph_peaks: pairs %lld edges %lld passes %d merge_ms %.3f waits_ms %.3f %.3f %.3f merged_ms %.3f\n", (long long)T,
                (long long)E, passes, merge_ms, at_pairs, at_edges, at_list, at_merged);
    SPH_HIP(hipMemsetAsync(top, 0xff, (size_t)no * sizeof(int32_t), st));          // no entry: a peak is its own top
    SPH_HIP(hipMemsetAsync(npk, 0, (size_t)no * sizeof(int32_t), st));
    SPH_HIP(hipMemsetAsync(minid, 0x7f, (size_t)no * sizeof(int32_t), st));
    SPH_HIP(hipMemsetAsync(rtop, 0xff, (size_t)no * sizeof(int32_t), st));
    SPH_HIP(hipMemsetAsync(sout, 0, (size_t)no * sizeof(double), st));
    if (E > 0) {
        SPH_HIP(hipMemcpyAsync(up_tops, m_tops.data(), (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, st));
        SPH_HIP(hipMemcpyAsync(up_sout, m_sout.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice, st));
        peaks_scatter<<<dim3(blocks(P, PB)), dim3(PB), 0, st>>>(plist, up_tops, up_sout, P, no, top, sout);
    }
    peaks_assign<<<dim3(blocks(no, PB)), dim3(PB), 0, st>>>(w.parent, top, rho, inv_slot, no, d->peak_min, w.info, npk);
    peaks_minid<<<dim3(blocks(no, PB)), dim3(PB), 0, st>>>(w.parent, no, minid);
    peaks_root<<<dim3(blocks(no, PB)), dim3(PB), 0, st>>>(w.parent, minid, no, rtop);
    SPH_HIP(hipGetLastError());
    if (E > 0) SPH_HIP(hipStreamSynchronize(st));                     // the uploads read the vectors above (pageable memory)
    int32_t *d_labels = labels ? (host ? h_labels : labels) : nullptr;
    double *d_table = host ? h_table : table;
    int64_t *d_counts = host ? d_counts_own : counts;
    SPH_TRY(groups_tail(c, w, d->min_members, d_labels, rows > 0 ? t21 : nullptr));
    peaks_table<<<dim3(blocks(rows, PB)), dim3(PB), 0, st>>>(t21, rows, w.info, pinfo, pidx + no, rtop, sout, npk, no, d_table, d_counts);
    SPH_HIP(hipGetLastError());
    if (!host) return SPH_OK;
    // host form: the counts, the labels and the table rows in one read-back
    std::vector<double> trow((size_t)rows * SPH_PEAKS_NCOL);
    SPH_HIP(hipMemcpyAsync(c->rnd_pinned, d_counts, SPH_PEAKS_NCOUNT * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (labels && n > 0) SPH_HIP(hipMemcpyAsync(labels, d_labels, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (rows > 0) SPH_HIP(hipMemcpyAsync(trow.data(), d_table, trow.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    int64_t hc[SPH_PEAKS_NCOUNT];
    std::memcpy(hc, c->rnd_pinned, sizeof hc);
    if (hc[0] < 0) {
        c->err = "sph_peaks: SPH_PEAKS_LINK_H: a selected particle has h <= 0 or a non-finite h";
        return SPH_ERR_STATE;
    }
    std::memcpy(counts, hc, sizeof hc);
    if (rows > 0) std::memcpy(table, trow.data(), (size_t)std::min(hc[0], rows) * SPH_PEAKS_NCOL * sizeof(double));
    return SPH_OK;
}

}  // namespace sph
