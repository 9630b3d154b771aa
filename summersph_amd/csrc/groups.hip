// groups.hip -- friends-of-friends groups (clumps) of the owned gas: the connected components of the graph that links
// every two selected particles closer than a linking length (include/summersph.h, sph_groups).
//
// Not part of the step loop: nothing here reads or writes the context's grid, cell table, neighbour list, statistics or
// flags.  The scratch is the one the analysis calls share (analysis_scratch).
//
// Pipeline (all on ctx->stream; counts, box and cell edge stay on the device):
//   groups_select    every slot: the selection; parent[id] = id (selected) or -1, count 0, number -1; per-block box, h_max,
//                    count and bad-h partials
//   groups_box       one wavefront: box, h_max, count -> the cell edge E = b_max (1 + 1e-6), enlarged where an axis would
//                    need more than 2^21 - 8 cells; no selected particle is processed when a selected h is bad (LINK_H)
//   groups_keys      every slot: the 63-bit cell key cx << 42 | cy << 21 | cz (selected) or ~0 (sorts behind every cell)
//   rocprim radix sort (cell key, slot)
//   groups_gather    sorted position p < count: {x, y, z, h} and the original id in sorted order; the first position of
//                    every cell puts {key, start} into an open-addressing hash table (atomicCAS on the key)
//   groups_tails     the last position of every cell writes its end into the cell's entry
//   groups_link      one lane per sorted position p: the own cell and its 13 neighbours of larger key (pairs q > p only),
//                    found through the hash table; linked pairs are joined in a lock-free union-find (below)
//   groups_jump      rounds of in-place pointer jumping (each lane follows up to JUMP links): parent[id] = the root
//   groups_count     integer atomics: members per root
//   groups_root_keys / rocprim radix sort / groups_number: roots with >= min_members members by (N descending, root id)
//                    -> group numbers 0 .. n_groups - 1, n_groups on the device
//   groups_members   every slot: member key (group << 32 | id) or ~0, and the label of its id
//   rocprim radix sort (group, id)
//   groups_starts    start[g] = first sorted position of group g, start[n_groups] = members
//   groups_pieces<1> / groups_final<1>: N, M, sum m r, sum m v, sum m u per group in the fixed shape of profile.hip
//                    (pieces of 1024 sorted positions from the group's start, one wavefront each, then one wavefront per
//                    group); R = sum m r / M and V = sum m v / M stay on the device
//   groups_pieces<2> / groups_final<2>: the moments about R and V, r_max, rho_max and its member -> the table rows
// groups_select .. groups_tails are the host function groups_front and groups_count .. groups_final the host function
// groups_tail (sph_internal.hpp): sph_peaks (peaks.hip) runs the same two around its own partition.
//
// Union-find (groups_link).  parent[] is indexed by original id and every link points to a smaller id, so a root is the
// smallest id of its tree and no cycle can form.  A find follows parent links with plain loads; such a load may return an
// older value (another CU's L1 or another XCD's L2 can hold a stale line), but every value parent[x] ever held is an id of
// x's component that is <= x, so a find always ends, at a node of the right component.  Joining roots a > b is one
// atomicCAS(&parent[a], a, b): it succeeds only while a is still a root (checked by the atomic itself, never by a plain
// load) and a failed CAS continues from the value it returned, which is < a; so each retry lowers max(a, b) and the loop
// ends.  Two finds that return the same node prove the pair already connected, whatever their staleness, and skip the CAS.
// Path halving lowers parent[x] with atomicMin to an ancestor: a value that only ever decreases, never on a root.  Nothing
// depends on a plain load seeing a store of the same launch; the flattening (groups_jump) is a separate launch.  The
// partition, and with it every label and table entry, is therefore independent of the schedule.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cell_table.hpp"
#include "reduce_common.hpp"

// the predicate and the per-particle arithmetic are written in one documented order (summersph.h); no contraction into
// fused multiply-adds, so that the numpy restatement reproduces them bit for bit
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int GB = 256;                    // block of the per-slot kernels
constexpr int BOX_BLOCKS = 1024;           // select blocks at most (grid-stride beyond)
constexpr int NP1 = 8;                     // first pass: M, sum m r (3), sum m v (3), sum m u
constexpr int NP2 = 9;                     // second pass: sum m d2, spin (3), K_int, r_max, rho_max, its id, its slot
constexpr int NGS = 9;                     // per group after the first pass: N, M, R (3), V (3), U
constexpr int JUMP = 16;                   // links a lane follows per jump round
constexpr int COUNT_RUN = 16;              // consecutive ids per thread of groups_count

using Sel = GroupsSel;                     // sph_internal.hpp: shared with peaks.hip
using Info = GroupsInfo;

__device__ __forceinline__ bool selected(const Sel &s, double x, double y, double z, double rho) {
    return rho >= s.rho_min && rho <= s.rho_cap && s.clip_lo[0] < x && x < s.clip_hi[0] && s.clip_lo[1] < y && y < s.clip_hi[1] &&
           s.clip_lo[2] < z && z < s.clip_hi[2];
}

__device__ __forceinline__ double h_of(const Sel &s, int64_t i) { return s.hf ? s.hf[i] : s.fixed_h; }

// parent[id] for every owned id, the per-block partials lo (3), hi (3), h_max, count, bad
__global__ __launch_bounds__(GB) void groups_select(const double *__restrict__ x, const double *__restrict__ y,
                                                    const double *__restrict__ z, const double *__restrict__ rho,
                                                    const int32_t *__restrict__ orig, int64_t n_slots, int64_t n_owned, Sel s,
                                                    int32_t *__restrict__ parent, int32_t *__restrict__ cnt,
                                                    int32_t *__restrict__ gnum, double *__restrict__ part) {
    __shared__ double red[9][GB];
    double v[9] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * GB) {
        const int32_t id = orig[i];
        if (id >= n_owned) continue;                    // ghosts and replaced ghosts
        const double px = x[i], py = y[i], pz = z[i];
        const bool sel = selected(s, px, py, pz, rho[i]);
        parent[id] = sel ? id : -1;
        cnt[id] = 0;
        gnum[id] = -1;
        if (!sel) continue;
        v[0] = fmin(v[0], px); v[1] = fmin(v[1], py); v[2] = fmin(v[2], pz);
        v[3] = fmax(v[3], px); v[4] = fmax(v[4], py); v[5] = fmax(v[5], pz);
        v[7] += 1.0;
        if (s.link_h) {
            const double h = h_of(s, i);
            if (h > 0.0 && h <= 1.7976931348623157e308) v[6] = fmax(v[6], h);
            else v[8] = 1.0;
        }
    }
    for (int a = 0; a < 9; a++) red[a][threadIdx.x] = v[a];
    __syncthreads();
    for (int w = GB / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            for (int a = 0; a < 3; a++) red[a][threadIdx.x] = fmin(red[a][threadIdx.x], red[a][threadIdx.x + w]);
            for (int a = 3; a < 7; a++) red[a][threadIdx.x] = fmax(red[a][threadIdx.x], red[a][threadIdx.x + w]);
            red[7][threadIdx.x] += red[7][threadIdx.x + w];
            red[8][threadIdx.x] = fmax(red[8][threadIdx.x], red[8][threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 9) part[blockIdx.x * 9 + threadIdx.x] = red[threadIdx.x][0];
}

// one wavefront: the partials -> Info (box, cell edge, count)
__global__ __launch_bounds__(WAVE) void groups_box(const double *__restrict__ part, int nb, Sel s, Info *__restrict__ info) {
    const int lane = threadIdx.x;
    double v[9] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0, 0.0, 0.0};
    for (int b = lane; b < nb; b += WAVE) {
        for (int a = 0; a < 3; a++) v[a] = fmin(v[a], part[b * 9 + a]);
        for (int a = 3; a < 7; a++) v[a] = fmax(v[a], part[b * 9 + a]);
        v[7] += part[b * 9 + 7];
        v[8] = fmax(v[8], part[b * 9 + 8]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        for (int a = 0; a < 3; a++) v[a] = fmin(v[a], __shfl_xor(v[a], o, 64));
        for (int a = 3; a < 7; a++) v[a] = fmax(v[a], __shfl_xor(v[a], o, 64));
        v[7] += __shfl_xor(v[7], o, 64);            // integer counts: exact in any order
        v[8] = fmax(v[8], __shfl_xor(v[8], o, 64));
    }
    if (lane != 0) return;
    const bool bad = v[8] != 0.0;
    double e = (s.link_h ? s.link * v[6] : s.link) * (1.0 + 1e-6);
    for (int a = 0; a < 3; a++) {
        const double ext = v[3 + a] - v[a];
        if (ext / e > AXIS_CELLS) e = (ext / AXIS_CELLS) * (1.0 + 1e-6);
    }
    for (int a = 0; a < 3; a++) info->lo[a] = v[a];
    info->inv_e = 1.0 / e;
    info->n_sel = bad ? 0 : (int64_t)v[7];
    info->n_groups = bad ? -1 : 0;
    info->bad = bad ? 1 : 0;
}

__global__ __launch_bounds__(GB) void groups_keys(const double *__restrict__ x, const double *__restrict__ y,
                                                  const double *__restrict__ z, const double *__restrict__ rho,
                                                  const int32_t *__restrict__ orig, int64_t n_slots, int64_t n_owned, Sel s,
                                                  const Info *__restrict__ info, uint64_t *__restrict__ keys,
                                                  uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (i >= n_slots) return;
    uint64_t key = ~0ull;
    if (orig[i] < n_owned && info->n_sel > 0) {
        const double px = x[i], py = y[i], pz = z[i];
        if (selected(s, px, py, pz, rho[i])) key = cell_key(px, py, pz, info->lo, info->inv_e);
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

// {x, y, z, h} and the original id in sorted order; every cell's first position enters the table
__global__ __launch_bounds__(GB) void groups_gather(const double *__restrict__ x, const double *__restrict__ y,
                                                    const double *__restrict__ z, const int32_t *__restrict__ orig, Sel s,
                                                    const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sval,
                                                    const Info *__restrict__ info, int64_t n_slots, double4 *__restrict__ rec,
                                                    int32_t *__restrict__ sid, Ent *__restrict__ tab, uint64_t mask) {
    const int64_t p = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (p >= n_slots || p >= info->n_sel) return;
    const uint32_t i = sval[p];
    rec[p] = make_double4(x[i], y[i], z[i], h_of(s, i));
    sid[p] = orig[i];
    cell_enter(skey, p, tab, mask);
}

__global__ __launch_bounds__(GB) void groups_tails(const uint64_t *__restrict__ skey, const Info *__restrict__ info, int64_t n_slots,
                                                   Ent *__restrict__ tab, uint64_t mask) {
    cell_close(skey, (int64_t)blockIdx.x * GB + threadIdx.x, n_slots, info->n_sel, tab, mask);
}

// the node a chain of parent links from x ends at (plain loads: possibly an older root of x's tree, see the top); every
// second link is shortened to the grandparent with an atomicMin once the chain is three links long
__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t x) {
    while (true) {
        const int32_t p = parent[x];
        if (p == x) return x;
        const int32_t g = parent[p];
        if (g == p) return p;
        const int32_t gg = parent[g];
        if (gg == g) return g;
        atomicMin(&parent[x], g);
        x = g;
    }
}

// joins the trees of a and b; returns an ancestor of both (the root b ended under, or the common node found)
__device__ __forceinline__ int32_t uf_union(int32_t *parent, int32_t a, int32_t b) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    while (a != b) {
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicCAS(&parent[a], a, b);          // a > b: hook the larger root under the smaller
        if (old == a) return b;
        a = uf_find(parent, old);                                 // a was no root any more: go on from its fresh parent
        b = uf_find(parent, b);
    }
    return a;
}

__global__ __launch_bounds__(GB) void groups_link(const double4 *__restrict__ rec, const int32_t *__restrict__ sid,
                                                  const uint64_t *__restrict__ skey, const Info *__restrict__ info,
                                                  int64_t n_slots, const Ent *__restrict__ tab, uint64_t mask, double link,
                                                  double b2, int32_t link_h, int32_t *parent) {
    const int64_t p = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (p >= n_slots || p >= info->n_sel) return;
    const double4 r = rec[p];
    const uint64_t key = skey[p];
    const int64_t c[3] = {(int64_t)(key >> (2 * AXIS_BITS)), (int64_t)((key >> AXIS_BITS) & AXIS_MASK), (int64_t)(key & AXIS_MASK)};
    int32_t root = sid[p];
    // offsets 13 .. 26 of the 27 (dx, dy, dz) in row-major order: the own cell (13) and the 13 cells of larger key
    for (int o = 13; o < 27; o++) {
        const int64_t n0 = c[0] + o / 9 - 1, n1 = c[1] + (o / 3) % 3 - 1, n2 = c[2] + o % 3 - 1;
        if (n0 < 0 || n1 < 0 || n2 < 0 || n0 > (int64_t)AXIS_MASK || n1 > (int64_t)AXIS_MASK || n2 > (int64_t)AXIS_MASK) continue;
        const uint64_t nk = ((uint64_t)n0 << (2 * AXIS_BITS)) | ((uint64_t)n1 << AXIS_BITS) | (uint64_t)n2;
        const int64_t t = hash_slot(tab, mask, nk);
        if (t < 0) continue;
        const int64_t q0 = o == 13 ? p + 1 : tab[t].start, q1 = tab[t].end;
        for (int64_t q = q0; q < q1; q++) {
            const double4 s = rec[q];
            const double dx = r.x - s.x, dy = r.y - s.y, dz = r.z - s.z;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            double bb = b2;
            if (link_h) {
                const double b = link * fmax(r.w, s.w);
                bb = b * b;
            }
            if (d2 < bb) root = uf_union(parent, root, sid[q]);
        }
    }
}

// one round of pointer jumping: parent[x] = the node JUMP links up (or the root).  Rounds are separate launches.
__global__ __launch_bounds__(GB) void groups_jump(int32_t *parent, int64_t n_owned) {
    const int64_t x = (int64_t)blockIdx.x * GB + threadIdx.x;
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

// members per root.  One hot address per large group: each thread counts COUNT_RUN consecutive ids, keeping its first
// root's count in a register (flushed once, summed over the wavefront for lane 0's root) and flushing other roots when they
// change, so a group that holds most particles sees about one atomic per wavefront instead of one per member
__global__ __launch_bounds__(GB) void groups_count(const int32_t *__restrict__ parent, int64_t n_owned, int32_t *__restrict__ cnt) {
    const int64_t x0 = ((int64_t)blockIdx.x * GB + threadIdx.x) * COUNT_RUN;
    const int lane = threadIdx.x & 63;
    int32_t a = -1, b = -1, ca = 0, cb = 0;
    for (int k = 0; k < COUNT_RUN; k++) {
        const int64_t x = x0 + k;
        const int32_t r = x < n_owned ? parent[x] : -1;
        if (r < 0) continue;
        if (a < 0) a = r;
        if (r == a) { ca++; continue; }
        if (r != b) {
            if (b >= 0) atomicAdd(&cnt[b], cb);
            b = r; cb = 0;
        }
        cb++;
    }
    if (b >= 0) atomicAdd(&cnt[b], cb);
    const int32_t a0 = __shfl(a, 0, 64);
    int32_t part = (a >= 0 && a == a0) ? ca : 0;
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);        // integers: exact in any order
    if (a >= 0 && a != a0) atomicAdd(&cnt[a], ca);
    if (lane == 0 && a0 >= 0) atomicAdd(&cnt[a0], part);
}

// roots with >= min_members members: (2^31 - 1 - N) << 32 | id, so that N descending, then the id, sort first
__global__ __launch_bounds__(GB) void groups_root_keys(const int32_t *__restrict__ parent, const int32_t *__restrict__ cnt,
                                                       int64_t n_owned, int64_t min_members, const Info *__restrict__ info,
                                                       uint64_t *__restrict__ keys) {
    const int64_t x = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (x >= n_owned) return;
    uint64_t key = ~0ull;
    if (info->n_groups >= 0 && parent[x] == x && (int64_t)cnt[x] >= min_members)
        key = ((uint64_t)(0x7fffffff - cnt[x]) << 32) | (uint64_t)x;
    keys[x] = key;
}

__global__ __launch_bounds__(GB) void groups_number(const uint64_t *__restrict__ rkey, int64_t n_owned, int32_t *__restrict__ gnum,
                                                    Info *__restrict__ info) {
    const int64_t g = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (g >= n_owned) return;
    const uint64_t k = rkey[g];
    if (k == ~0ull) return;
    gnum[k & 0xffffffffull] = (int32_t)g;
    if (g + 1 == n_owned || rkey[g + 1] == ~0ull) info->n_groups = g + 1;
}

// member keys (group << 32 | id) of every slot and the label of every owned id
__global__ __launch_bounds__(GB) void groups_members(const int32_t *__restrict__ orig, int64_t n_slots, int64_t n_owned,
                                                     const int32_t *__restrict__ parent, const int32_t *__restrict__ gnum,
                                                     uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                     int32_t *__restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (i >= n_slots) return;
    const int32_t id = orig[i];
    uint64_t key = ~0ull;
    if (id < n_owned) {
        const int32_t r = parent[id];
        const int32_t g = r >= 0 ? gnum[r] : -1;
        if (g >= 0) key = ((uint64_t)g << 32) | (uint64_t)(uint32_t)id;
        if (labels) labels[id] = g;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(GB) void groups_starts(const uint64_t *__restrict__ keys, int64_t n_slots, int32_t *__restrict__ start) {
    const int64_t p = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (p >= n_slots) return;
    const uint64_t k = keys[p];
    if (k == ~0ull) return;
    const int64_t g = (int64_t)(k >> 32);
    if (p == 0 || (keys[p - 1] >> 32) != (uint64_t)g) start[g] = (int32_t)p;
    if (p + 1 == n_slots || keys[p + 1] == ~0ull) start[g + 1] = (int32_t)(p + 1);
}

// the densest member: larger rho, then the smaller id (order-free)
__device__ __forceinline__ void best_of(double &rho, double &id, double &slot, double rho2, double id2, double slot2) {
    if (rho2 > rho || (rho2 == rho && id2 < id)) { rho = rho2; id = id2; slot = slot2; }
}

struct Fields { const double *x, *y, *z, *vx, *vy, *vz, *u, *m, *rho; const int32_t *orig; };

// one wavefront per piece slot; PASS 1: M, sum m r, sum m v, sum m u; PASS 2: the moments about R, V and the maxima
template <int PASS>
__global__ __launch_bounds__(GB) void groups_pieces(Fields f, const uint32_t *__restrict__ vals, const int32_t *__restrict__ start,
                                                    const Info *__restrict__ info, int64_t n_pieces, const double *__restrict__ gstat,
                                                    double *__restrict__ part) {
    constexpr int NP = PASS == 1 ? NP1 : NP2;
    const int64_t w = (int64_t)blockIdx.x * (GB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t ng = info->n_groups;
    if (w >= n_pieces || ng <= 0 || w > start[ng] / PIECE + ng) return;     // past the last piece slot in use
    int64_t g, p0, p1;
    if (!piece_locate(start, ng, w, g, p0, p1)) return;
    double acc[NP];
#pragma unroll
    for (int s = 0; s < NP; s++) acc[s] = 0.0;
    if (PASS == 1) {
        for (int64_t p = p0 + lane; p < p1; p += WAVE) {
            const uint32_t i = vals[p];
            const double m = f.m[i];
            const double q[NP1] = {m, m * f.x[i], m * f.y[i], m * f.z[i], m * f.vx[i], m * f.vy[i], m * f.vz[i], m * f.u[i]};
#pragma unroll
            for (int s = 0; s < NP1; s++) acc[s] += q[s];
        }
#pragma unroll
        for (int s = 0; s < NP; s++) acc[s] = wave_sum(acc[s]);
    } else {
        const double *G = gstat + g * NGS;
        const double R[3] = {G[2], G[3], G[4]}, V[3] = {G[5], G[6], G[7]};
        acc[6] = -INFINITY; acc[7] = INFINITY; acc[8] = -1.0;     // rho_max, its id, its slot
        for (int64_t p = p0 + lane; p < p1; p += WAVE) {
            const uint32_t i = vals[p];
            const double m = f.m[i];
            const double dr[3] = {f.x[i] - R[0], f.y[i] - R[1], f.z[i] - R[2]};
            const double dv[3] = {f.vx[i] - V[0], f.vy[i] - V[1], f.vz[i] - V[2]};
            const double d2 = (dr[0] * dr[0] + dr[1] * dr[1]) + dr[2] * dr[2];
            acc[0] += m * d2;
            acc[1] += m * (dr[1] * dv[2] - dr[2] * dv[1]);
            acc[2] += m * (dr[2] * dv[0] - dr[0] * dv[2]);
            acc[3] += m * (dr[0] * dv[1] - dr[1] * dv[0]);
            acc[4] += (0.5 * m) * ((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]);
            acc[5] = fmax(acc[5], sqrt(d2));
            best_of(acc[6], acc[7], acc[8], f.rho[i], (double)f.orig[i], (double)i);
        }
#pragma unroll
        for (int s = 0; s < 5; s++) acc[s] = wave_sum(acc[s]);
        for (int o = 32; o > 0; o >>= 1) {
            acc[5] = fmax(acc[5], __shfl_xor(acc[5], o, 64));
            best_of(acc[6], acc[7], acc[8], __shfl_xor(acc[6], o, 64), __shfl_xor(acc[7], o, 64), __shfl_xor(acc[8], o, 64));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NP; s++) part[w * NP + s] = acc[s];
    }
}


// one wavefront per group: its pieces in a fixed shape.  PASS 1 -> gstat[g] = {N, M, R, V, U}; PASS 2 -> table row g
// (g < rows)
template <int PASS>
__global__ __launch_bounds__(GB) void groups_final(const int32_t *__restrict__ start, const Info *__restrict__ info, int64_t n_bound,
                                                   const double *__restrict__ part, const uint64_t *__restrict__ mkey, Fields f,
                                                   double *__restrict__ gstat, double *__restrict__ table, int64_t rows) {
    constexpr int NP = PASS == 1 ? NP1 : NP2;
    const int64_t g = (int64_t)blockIdx.x * (GB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_bound || g >= info->n_groups) return;
    if (PASS == 2 && g >= rows) return;
    const int64_t len = (int64_t)start[g + 1] - start[g];
    const int64_t np = (len + PIECE - 1) / PIECE, base = piece_base(start, g);
    double acc[NP];
#pragma unroll
    for (int s = 0; s < NP; s++) acc[s] = 0.0;
    if (PASS == 2) { acc[5] = 0.0; acc[6] = -INFINITY; acc[7] = INFINITY; acc[8] = -1.0; }
    for (int64_t k = lane; k < np; k += WAVE) {
        const double *q = part + (base + k) * NP;
        const int ns = PASS == 1 ? NP1 : 5;
        for (int s = 0; s < ns; s++) acc[s] += q[s];
        if (PASS == 2) {
            acc[5] = fmax(acc[5], q[5]);
            best_of(acc[6], acc[7], acc[8], q[6], q[7], q[8]);
        }
    }
    if (PASS == 1) {
#pragma unroll
        for (int s = 0; s < NP; s++) acc[s] = wave_sum(acc[s]);
    } else {
#pragma unroll
        for (int s = 0; s < 5; s++) acc[s] = wave_sum(acc[s]);
        for (int o = 32; o > 0; o >>= 1) {
            acc[5] = fmax(acc[5], __shfl_xor(acc[5], o, 64));
            best_of(acc[6], acc[7], acc[8], __shfl_xor(acc[6], o, 64), __shfl_xor(acc[7], o, 64), __shfl_xor(acc[8], o, 64));
        }
    }
    if (lane != 0) return;
    double *G = gstat + g * NGS;
    if (PASS == 1) {
        const double M = acc[0];
        G[0] = (double)len;
        G[1] = M;
        for (int a = 0; a < 3; a++) { G[2 + a] = acc[1 + a] / M; G[5 + a] = acc[4 + a] / M; }
        G[8] = acc[7];
    } else {
        double *t = table + g * SPH_GROUPS_NCOL;
        const int64_t slot = (int64_t)acc[8];
        for (int s = 0; s < 8; s++) t[s] = G[s];
        t[8] = sqrt(acc[0] / G[1]);
        t[9] = acc[5];
        t[10] = acc[1]; t[11] = acc[2]; t[12] = acc[3];
        t[13] = acc[4];
        t[14] = G[8];
        t[15] = acc[6];
        t[16] = slot >= 0 ? f.x[slot] : NAN; t[17] = slot >= 0 ? f.y[slot] : NAN; t[18] = slot >= 0 ? f.z[slot] : NAN;
        t[19] = acc[7];
        t[20] = (double)(mkey[start[g]] & 0xffffffffull);      // members run in id order: the first is the smallest
    }
}

}  // namespace

void groups_sizes(const sph_ctx *c, int64_t min_members, int64_t max_groups, GroupsWork &w) {
    w.ns = c->cap > 0 ? c->n_slots : 0;
    w.no = c->n_owned;
    w.gb = w.no / min_members;                                   // groups there can be at most
    w.rows = std::min(max_groups, w.gb);                         // table rows written
    w.n_pieces = w.ns / PIECE + w.gb + 1;
    w.nb = (int)std::min<int64_t>((w.ns + GB - 1) / GB, BOX_BLOCKS);
    w.tl = 1;
    while (w.tl < 2 * w.ns) w.tl <<= 1;                          // hash table: load <= 1/2
    size_t sort_pairs = 0, sort_keys = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_pairs, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                    (uint32_t *)nullptr, (size_t)w.ns, 0u, 64u, c->stream);
    (void)rocprim::radix_sort_keys(nullptr, sort_keys, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)w.no, 0u, 64u, c->stream);
    w.sort_bytes = std::max(sort_pairs, sort_keys);
}

void groups_take(GroupsWork &w, Carve &cv) {
    const int64_t ns = w.ns, no = w.no;
    w.keys = cv.take<uint64_t>(ns);
    w.keys_alt = cv.take<uint64_t>(ns);
    w.vals = cv.take<uint32_t>(ns);
    w.vals_alt = cv.take<uint32_t>(ns);
    w.sort_tmp = cv.take<char>(w.sort_bytes);
    w.rec = cv.take<double4>(ns);
    w.sid = cv.take<int32_t>(ns);
    w.tab = cv.take<Ent>(w.tl);
    w.parent = cv.take<int32_t>(no);
    w.cnt = cv.take<int32_t>(no);
    w.gnum = cv.take<int32_t>(no);
    w.box_part = cv.take<double>(9 * (size_t)w.nb);
    w.info = cv.take<Info>(1);
    w.start = cv.take<int32_t>(w.gb + 1);
    w.part = cv.take<double>(NP2 * (size_t)w.n_pieces);
    w.gstat = cv.take<double>(NGS * (size_t)std::max<int64_t>(w.gb, 1));
}

int groups_front(sph_ctx *c, const GroupsSel &s, GroupsWork &w) {
    hipStream_t st = c->stream;
    const int64_t ns = w.ns, no = w.no;
    const double *x = c->f[SPH_F_X], *y = c->f[SPH_F_Y], *z = c->f[SPH_F_Z], *rho = c->f[SPH_F_RHO];
    // selection, box, cell edge
    groups_select<<<dim3((unsigned)w.nb), dim3(GB), 0, st>>>(x, y, z, rho, c->orig, ns, no, s, w.parent, w.cnt, w.gnum, w.box_part);
    groups_box<<<dim3(1), dim3(WAVE), 0, st>>>(w.box_part, w.nb, s, w.info);
    SPH_HIP(hipGetLastError());
    // cell keys, sort, hash table over the occupied cells
    groups_keys<<<dim3(blocks(ns, GB)), dim3(GB), 0, st>>>(x, y, z, rho, c->orig, ns, no, s, w.info, w.keys, w.vals);
    size_t tmp = w.sort_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(w.sort_tmp, tmp, w.keys, w.keys_alt, w.vals, w.vals_alt, (size_t)ns, 0u, 64u, st));
    SPH_HIP(hipMemsetAsync(w.tab, 0xff, sizeof(Ent) * (size_t)w.tl, st));
    groups_gather<<<dim3(blocks(ns, GB)), dim3(GB), 0, st>>>(x, y, z, c->orig, s, w.keys_alt, w.vals_alt, w.info, ns, w.rec, w.sid,
                                                              w.tab, (uint64_t)(w.tl - 1));
    groups_tails<<<dim3(blocks(ns, GB)), dim3(GB), 0, st>>>(w.keys_alt, w.info, ns, w.tab, (uint64_t)(w.tl - 1));
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

int groups_tail(sph_ctx *c, GroupsWork &w, int64_t min_members, int32_t *d_labels, double *d_table) {
    hipStream_t st = c->stream;
    const int64_t n = c->n, ns = w.ns, no = w.no, gb = w.gb, rows = w.rows, n_pieces = w.n_pieces;
    const double *x = c->f[SPH_F_X], *y = c->f[SPH_F_Y], *z = c->f[SPH_F_Z], *rho = c->f[SPH_F_RHO];
    groups_count<<<dim3(blocks((no + COUNT_RUN - 1) / COUNT_RUN, GB)), dim3(GB), 0, st>>>(w.parent, no, w.cnt);
    // numbering: (N descending, root id)
    groups_root_keys<<<dim3(blocks(no, GB)), dim3(GB), 0, st>>>(w.parent, w.cnt, no, min_members, w.info, w.keys);
    size_t tmp = w.sort_bytes;
    SPH_HIP(rocprim::radix_sort_keys(w.sort_tmp, tmp, w.keys, w.keys_alt, (size_t)no, 0u, 64u, st));
    groups_number<<<dim3(blocks(no, GB)), dim3(GB), 0, st>>>(w.keys_alt, no, w.gnum, w.info);
    // members in (group, id) order, labels
    if (d_labels && n > no) SPH_HIP(hipMemsetAsync(d_labels + no, 0xff, (size_t)(n - no) * sizeof(int32_t), st));   // ghosts
    groups_members<<<dim3(blocks(ns, GB)), dim3(GB), 0, st>>>(c->orig, ns, no, w.parent, w.gnum, w.keys, w.vals, d_labels);
    tmp = w.sort_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(w.sort_tmp, tmp, w.keys, w.keys_alt, w.vals, w.vals_alt, (size_t)ns, 0u, 64u, st));
    groups_starts<<<dim3(blocks(ns, GB)), dim3(GB), 0, st>>>(w.keys_alt, ns, w.start);
    SPH_HIP(hipGetLastError());
    // the two reductions
    Fields f{x, y, z, c->f[SPH_F_VX], c->f[SPH_F_VY], c->f[SPH_F_VZ], c->f[SPH_F_U], c->f[SPH_F_M], rho, c->orig};
    const int wpb = GB / WAVE;
    groups_pieces<1><<<dim3(blocks(n_pieces, wpb)), dim3(GB), 0, st>>>(f, w.vals_alt, w.start, w.info, n_pieces, w.gstat, w.part);
    groups_final<1><<<dim3(blocks(gb, wpb)), dim3(GB), 0, st>>>(w.start, w.info, gb, w.part, w.keys_alt, f, w.gstat, d_table, rows);
    if (rows > 0) {
        groups_pieces<2><<<dim3(blocks(n_pieces, wpb)), dim3(GB), 0, st>>>(f, w.vals_alt, w.start, w.info, n_pieces, w.gstat, w.part);
        groups_final<2><<<dim3(blocks(rows, wpb)), dim3(GB), 0, st>>>(w.start, w.info, gb, w.part, w.keys_alt, f, w.gstat, d_table, rows);
    }
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

int groups_run(sph_ctx *c, const sph_groups_desc *d, int32_t *labels, int64_t n_labels, double *table, int64_t max_groups,
               int64_t *n_groups, bool host) {
    const char *who = "sph_groups";
    if (!d) return arg_error(c, who, "null descriptor");
    if (!n_groups) return arg_error(c, who, "null count pointer");
    if (d->reserved != 0) return arg_error(c, who, "reserved must be 0");
    if (d->flags & ~SPH_GROUPS_LINK_H) return arg_error(c, who, "unknown flags");
    if (!(d->link > 0.0) || !std::isfinite(d->link)) return arg_error(c, who, "link must be finite and > 0");
    if (std::isnan(d->rho_min)) return arg_error(c, who, "rho_min is NaN");
    for (int a = 0; a < 3; a++)
        if (std::isnan(d->clip_lo[a]) || std::isnan(d->clip_hi[a])) return arg_error(c, who, "the clip box has a NaN");
    if (d->min_members < 1) return arg_error(c, who, "min_members must be >= 1");
    if (labels && n_labels != c->n) return arg_error(c, who, "n_labels != sph_count");
    if (max_groups < 0) return arg_error(c, who, "max_groups < 0");
    if (table && max_groups == 0) return arg_error(c, who, "a table needs max_groups > 0");
    if (!field_ready(*c, c->variable, SPH_F_RHO)) { c->err = "sph_groups: rho is stale (call sph_density)"; return SPH_ERR_STATE; }
    const bool link_h = (d->flags & SPH_GROUPS_LINK_H) != 0;
    if (link_h && !c->variable && !(c->p.h > 0.0 && std::isfinite(c->p.h))) {
        c->err = "sph_groups: SPH_GROUPS_LINK_H needs h > 0";
        return SPH_ERR_STATE;
    }

    hipStream_t st = c->stream;
    const int64_t n = c->n, no = c->n_owned;
    const int64_t ns = c->cap > 0 ? c->n_slots : 0;
    if (!table) max_groups = 0;
    if (ns == 0 || no == 0) {                       // nothing owned: no group, every label -1
        if (host) {
            if (labels) std::fill(labels, labels + n, -1);
            *n_groups = 0;
        } else {
            if (labels && n > 0) SPH_HIP(hipMemsetAsync(labels, 0xff, (size_t)n * sizeof(int32_t), st));
            SPH_HIP(hipMemsetAsync(n_groups, 0, sizeof(int64_t), st));
        }
        return SPH_OK;
    }
    GroupsWork w{};
    groups_sizes(c, d->min_members, max_groups, w);
    const int64_t rows = w.rows;
    int32_t *h_labels;
    double *h_table;
    auto layout = [&](Carve cv) {
        groups_take(w, cv);
        h_labels = cv.take<int32_t>(host && labels ? n : 0);                     // the host form's device copies
        h_table = cv.take<double>(host ? SPH_GROUPS_NCOL * (size_t)rows : 0);
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    int32_t *d_labels = labels ? (host ? h_labels : labels) : nullptr;
    double *d_table = host ? h_table : table;
    if (host) SPH_TRY(analysis_pinned(c));

    Sel s{};
    s.rho_min = d->rho_min;
    s.rho_cap = INFINITY;
    for (int a = 0; a < 3; a++) { s.clip_lo[a] = d->clip_lo[a]; s.clip_hi[a] = d->clip_hi[a]; }
    s.link = d->link;
    s.fixed_h = c->p.h;
    s.hf = c->variable ? c->f[SPH_F_H] : nullptr;
    s.link_h = link_h ? 1 : 0;
    const double b2 = d->link * d->link;
    SPH_TRY(groups_front(c, s, w));
    // links, then the flattening: every round multiplies the links a pointer spans by JUMP (>= 16^rounds >= no)
    groups_link<<<dim3(blocks(ns, GB)), dim3(GB), 0, st>>>(w.rec, w.sid, w.keys_alt, w.info, ns, w.tab, (uint64_t)(w.tl - 1), d->link,
                                                            b2, s.link_h, w.parent);
    SPH_HIP(hipGetLastError());
    int rounds = 1;
    for (double span = JUMP; span < (double)no; span *= JUMP) rounds++;
    for (int r = 0; r < rounds; r++) groups_jump<<<dim3(blocks(no, GB)), dim3(GB), 0, st>>>(w.parent, no);
    SPH_TRY(groups_tail(c, w, d->min_members, d_labels, d_table));
    const Info *info = w.info;
    if (!host) {
        SPH_HIP(hipMemcpyAsync(n_groups, &info->n_groups, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        return SPH_OK;
    }
    // host form: the count, the labels and the table rows in one read-back
    std::vector<double> trow((size_t)rows * SPH_GROUPS_NCOL);
    SPH_HIP(hipMemcpyAsync(c->rnd_pinned, &info->n_groups, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (labels && n > 0) SPH_HIP(hipMemcpyAsync(labels, d_labels, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (rows > 0) SPH_HIP(hipMemcpyAsync(trow.data(), d_table, trow.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    int64_t ng = 0;
    std::memcpy(&ng, c->rnd_pinned, sizeof(int64_t));
    if (ng < 0) {
        c->err = "sph_groups: SPH_GROUPS_LINK_H: a selected particle has h <= 0 or a non-finite h";
        return SPH_ERR_STATE;
    }
    *n_groups = ng;
    if (rows > 0) std::memcpy(table, trow.data(), (size_t)std::min(ng, rows) * SPH_GROUPS_NCOL * sizeof(double));
    return SPH_OK;
}

}  // namespace sph
