// bound.hip -- binding energies and unbinding of clumps: for every group of a caller's partition of the owned gas, the
// group's own softened potential by a direct pair sum in fp64, the energies of its members in the group's frame, and the
// iterated removal of the members with e >= 0 (include/summersph.h, sph_bound).
//
// Not part of the step loop: nothing here reads or writes the context's grid, cell table, neighbour list, statistics or
// flags.  The scratch is the one the analysis calls share (analysis_scratch).
//
// Pipeline (all on ctx->stream; every count and decision stays on the device):
//   bound_fill       the outputs' defaults: label -1, e and Phi NaN for every particle
//   bound_keys       every slot: the member key (group << 32 | id) of an owned particle with a finite position and a label
//                    in [0, n_groups), else ~0 (sorts last)
//   rocprim radix sort (key, slot): the members of a group in ascending original id, the groups in ascending number
//   bound_starts     start[g] = the first sorted position of group g (a binary search: empty groups get an empty range),
//                    start[n_groups] = the number of members
//   bound_gather     sorted position p: the 32-byte source record {x, y, z, G m}, {h, vx, vy, vz, u, m}, the id; alive = 1;
//                    a member h <= 0 or non-finite raises the bad flag
//   bound_init       every group: N_0 against min_members / max_members -> active, dissolved (2) or skipped (3); the rows
//                    of the groups that are never evaluated
//   per round r = 0 .. (a fixed sequence of launches; every kernel leaves at once when no group is active in round r):
//     bound_mom        a wavefront per piece of 1024 sorted positions of an active group: r > 0 first removes the members
//                      with !(e < 0) (alive = 0); N, M, sum m v of the set
//     bound_mom_final  a wavefront per active group: the pieces -> N_r, M, V
//     bound_plan       the round's work list: the tiles of 64 sorted positions that hold a live member of an active
//                      group (appended with an integer atomic; an item's results do not depend on its place in the list)
//     bound_pairs      a wavefront per work item, a lane per target: for every active group that has members in the tile,
//                      the group's members stream through LDS in tiles of 256 source records (a removed member as a
//                      zero-mass source); every lane reads the same LDS address in the same trip (a broadcast); Phi_i is
//                      one accumulation chain in ascending id, the own record excluded by its sorted position; then e_i
//     bound_sums       a wavefront per piece: K, U, W, sum m r, the count of e < 0 and the most bound member
//     bound_sums_final a wavefront per active group: the row of the table, and the decision: converged (0), stopped at
//                      max_rounds (1), dissolved (2), or one more round
//   bound_scatter    sorted position p: e and Phi of the last evaluation that included the member, and its label
//   bound_counts     members, groups skipped, dissolved, stopped at max_rounds (integer atomics)
//
// Scheduling.  The work item of the pair kernel is a tile of 64 consecutive sorted positions, not a group: a group of 10^5
// members spreads over 1563 wavefronts, and the 54 000 groups of about 20 members that friends-of-friends finds in a disc
// pack three to a wavefront (each run of a tile's positions that belongs to one group is served in turn, its lanes active,
// the others idle), instead of one launch slot each.  Removed members are masked, not compacted away: a dead source adds
// +-0 to a chain, which leaves every bit of it as it is, and a tile without a live member of an active group is not in
// the work list.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "pair_common.hpp"
#include "reduce_common.hpp"

// the per-member arithmetic is written in one documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int BB = 256;                    // block of the per-slot and per-piece kernels
constexpr int TILE = WAVE;                 // targets per work item of the pair kernel: one per lane
constexpr int SRC = 256;                   // source records per LDS tile (8 KB)
constexpr int NPA = 5;                     // bound_mom: N, M, sum m v (3)
constexpr int NPB = 10;                    // bound_sums: K, U, W, sum m r (3), count of e < 0, the smallest e, its id, spare
constexpr int NGS = 5;                     // per group and round: N, M, V (3)
constexpr int ACTIVE = -1;                 // status of a group that is still being evaluated
constexpr double DBL_BIG = 1.7976931348623157e308;

struct Cfg {
    double soft2, fixed_h;                 // fixed_h: the softening length of every member when hf is null
    const double *hf;                      // per-particle h (slot order) or null
    double G;
    int64_t n_owned, n_groups, min_members, max_members;
    int32_t max_rounds, thermal;
};

// per sorted position
struct Members {
    double4 *rec;                          // {x, y, z, G m}: the source record
    double *h, *vx, *vy, *vz, *u, *m;
    double *e, *phi;                       // of the last evaluation that included the member (NaN before the first)
    int32_t *id;
    uint8_t *alive;
};

// per group
struct Groups {
    int32_t *start;                        // n_groups + 1 sorted positions
    int32_t *status;                       // ACTIVE, or 0 .. 3
    int32_t *rounds;                       // R: removals so far
    double *stat;                          // NGS doubles: the set of the current round
};

__global__ __launch_bounds__(BB) void bound_fill(int64_t n, int32_t *__restrict__ labels, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (i >= n) return;
    if (labels) labels[i] = -1;
    if (out) { out[i] = NAN; out[n + i] = NAN; }
}

__global__ __launch_bounds__(BB) void bound_keys(const double *__restrict__ x, const double *__restrict__ y,
                                                 const double *__restrict__ z, const int32_t *__restrict__ orig, int64_t n_slots,
                                                 int64_t n_owned, int64_t n_groups, const int32_t *__restrict__ labels,
                                                 uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (i >= n_slots) return;
    const int32_t id = orig[i];
    uint64_t key = ~0ull;
    if (id >= 0 && id < n_owned) {                  // ghosts and replaced ghosts are never members
        const int32_t g = labels[id];
        if (g >= 0 && g < n_groups && fabs(x[i]) <= DBL_BIG && fabs(y[i]) <= DBL_BIG && fabs(z[i]) <= DBL_BIG)
            key = ((uint64_t)g << 32) | (uint64_t)(uint32_t)id;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

// start[g] = the first sorted position whose key is >= g << 32 (g == n_groups: the number of members)
__global__ __launch_bounds__(BB) void bound_starts(const uint64_t *__restrict__ skey, int64_t n_slots, int64_t n_groups,
                                                   int32_t *__restrict__ start) {
    const int64_t g = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (g > n_groups) return;
    const uint64_t want = (uint64_t)g << 32;
    int64_t lo = 0, hi = n_slots;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skey[mid] < want) lo = mid + 1; else hi = mid;
    }
    start[g] = (int32_t)lo;
}

struct Fields { const double *x, *y, *z, *vx, *vy, *vz, *u, *m; const int32_t *orig; };

__global__ __launch_bounds__(BB) void bound_gather(Fields f, Cfg cfg, const uint32_t *__restrict__ sval,
                                                   const int32_t *__restrict__ start, int64_t n_slots, Members mb,
                                                   int32_t *__restrict__ bad) {
    const int64_t p = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (p >= n_slots || p >= start[cfg.n_groups]) return;
    const uint32_t i = sval[p];
    const double m = f.m[i];
    const double h = cfg.hf ? cfg.hf[i] : cfg.fixed_h;
    mb.rec[p] = make_double4(f.x[i], f.y[i], f.z[i], cfg.G * m);
    mb.h[p] = h;
    mb.vx[p] = f.vx[i]; mb.vy[p] = f.vy[i]; mb.vz[p] = f.vz[i];
    mb.u[p] = f.u[i];
    mb.m[p] = m;
    mb.e[p] = NAN; mb.phi[p] = NAN;
    mb.id[p] = f.orig[i];
    mb.alive[p] = 1;
    if (!(h > 0.0 && h <= DBL_BIG)) atomicOr(bad, 1);
}

__device__ __forceinline__ void row_unevaluated(double *t, double n0, int status) {
    for (int c = 0; c < SPH_BOUND_NCOL; c++) t[c] = NAN;
    t[0] = n0;
    t[21] = (double)status;
    if (status == 2) { t[7] = 0.0; t[8] = 0.0; t[19] = 0.0; t[20] = 0.0; t[22] = -1.0; }
}

// every group: active, dissolved before any evaluation, or skipped; act[0] counts the active ones
__global__ __launch_bounds__(BB) void bound_init(Cfg cfg, Groups gr, const int32_t *__restrict__ bad, double *__restrict__ table,
                                                 int32_t *__restrict__ act) {
    const int64_t g = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (g >= cfg.n_groups) return;
    const int64_t n0 = (int64_t)gr.start[g + 1] - gr.start[g];
    gr.rounds[g] = 0;
    if (*bad) {                                     // a member's h cannot be used: nothing is evaluated, every row is NaN
        gr.status[g] = 3;
        if (table)
            for (int c = 0; c < SPH_BOUND_NCOL; c++) table[g * SPH_BOUND_NCOL + c] = NAN;
        return;
    }
    const int st = n0 > cfg.max_members ? 3 : (n0 < cfg.min_members ? 2 : ACTIVE);
    gr.status[g] = st;
    if (st == ACTIVE) atomicAdd(&act[0], 1);
    else if (table) row_unevaluated(table + g * SPH_BOUND_NCOL, (double)n0, st);
}

// A wavefront per piece slot.  r > 0: the members of an active group whose last e is not < 0 leave the set first.
__global__ __launch_bounds__(BB) void bound_mom(Members mb, Groups gr, int64_t n_groups, int64_t n_pieces, int round,
                                                const int32_t *__restrict__ act, double *__restrict__ part) {
    if (act[round] == 0) return;
    const int64_t w = (int64_t)blockIdx.x * (BB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= n_pieces || w > gr.start[n_groups] / PIECE + n_groups) return;
    int64_t g, p0, p1;
    if (!piece_locate(gr.start, n_groups, w, g, p0, p1)) return;
    if (gr.status[g] != ACTIVE) return;
    double acc[NPA];
#pragma unroll
    for (int s = 0; s < NPA; s++) acc[s] = 0.0;
    for (int64_t p = p0 + lane; p < p1; p += WAVE) {
        if (!mb.alive[p]) continue;
        if (round > 0 && !(mb.e[p] < 0.0)) { mb.alive[p] = 0; continue; }
        const double m = mb.m[p];
        const double q[NPA] = {1.0, m, m * mb.vx[p], m * mb.vy[p], m * mb.vz[p]};
#pragma unroll
        for (int s = 0; s < NPA; s++) acc[s] += q[s];
    }
#pragma unroll
    for (int s = 0; s < NPA; s++) acc[s] = wave_sum(acc[s]);
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NPA; s++) part[w * NPA + s] = acc[s];
    }
}

__global__ __launch_bounds__(BB) void bound_mom_final(Groups gr, int64_t n_groups, int round, const int32_t *__restrict__ act,
                                                      const double *__restrict__ part) {
    if (act[round] == 0) return;
    const int64_t g = (int64_t)blockIdx.x * (BB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_groups || gr.status[g] != ACTIVE) return;
    const int64_t len = (int64_t)gr.start[g + 1] - gr.start[g];
    const int64_t np = (len + PIECE - 1) / PIECE, base = piece_base(gr.start, g);
    double acc[NPA];
#pragma unroll
    for (int s = 0; s < NPA; s++) acc[s] = 0.0;
    for (int64_t k = lane; k < np; k += WAVE) {
#pragma unroll
        for (int s = 0; s < NPA; s++) acc[s] += part[(base + k) * NPA + s];
    }
#pragma unroll
    for (int s = 0; s < NPA; s++) acc[s] = wave_sum(acc[s]);
    if (lane != 0) return;
    double *G = gr.stat + g * NGS;
    G[0] = acc[0];
    G[1] = acc[1];
    for (int a = 0; a < 3; a++) G[2 + a] = acc[2 + a] / acc[1];
}

// the tiles of TILE sorted positions that hold a live member of an active group -> list[0 .. n_list[round])
__global__ __launch_bounds__(BB) void bound_plan(Members mb, Groups gr, const uint64_t *__restrict__ skey, int64_t n_groups,
                                                 int64_t n_tiles, int round, const int32_t *__restrict__ act,
                                                 int32_t *__restrict__ list, int32_t *__restrict__ n_list) {
    if (act[round] == 0) return;
    const int64_t t = (int64_t)blockIdx.x * BB + threadIdx.x;
    const int64_t members = gr.start[n_groups];
    if (t >= n_tiles || t * TILE >= members) return;
    const int64_t end = min(members, (t + 1) * TILE);
    bool any = false;
    for (int64_t pos = t * TILE; pos < end && !any;) {
        const int64_t g = (int64_t)(skey[pos] >> 32);
        const int64_t run_end = min(end, (int64_t)gr.start[g + 1]);
        if (gr.status[g] == ACTIVE)
            for (int64_t p = pos; p < run_end && !any; p++) any = mb.alive[p] != 0;
        pos = run_end;
    }
    if (any) list[atomicAdd(&n_list[round], 1)] = (int32_t)t;
}

// phi(q) of sph_energy's softening (gravity.hip, soft_phi): rq = 1 / q, used for q >= 1 only
__device__ __forceinline__ double bound_phi(double q, double rq) {
    const double q2 = q * q;
    if (q < 1.0) return q2 * ((2.0 / 3.0) + q2 * (-0.3 + 0.1 * q)) - 1.4;
    if (q < 2.0) return (q2 * ((4.0 / 3.0) + q * (-1.0 + q * (0.3 - q * (1.0 / 30.0)))) - 1.6) + rq * (1.0 / 15.0);
    return -rq;
}

// One wavefront per work item (a tile of 64 sorted positions), one target per lane.
__global__ __launch_bounds__(TILE) void bound_pairs(Members mb, Groups gr, const uint64_t *__restrict__ skey, int64_t n_groups,
                                                    double soft2, int thermal, int round, const int32_t *__restrict__ act,
                                                    const int32_t *__restrict__ list, const int32_t *__restrict__ n_list) {
    __shared__ double4 src[SRC];
    if (act[round] == 0 || (int)blockIdx.x >= n_list[round]) return;
    const int lane = threadIdx.x;
    const int64_t t = list[blockIdx.x];
    const int64_t members = gr.start[n_groups];
    const int64_t end = min(members, (t + 1) * TILE);
    const int64_t p = t * TILE + lane;
    const int64_t self = p < end ? p : end - 1;
    const double4 r = mb.rec[self];
    const double h = mb.h[self];
    const double inv_h = 1.0 / h;
    const bool live = p < end && mb.alive[self] != 0;
    for (int64_t pos = t * TILE; pos < end;) {                 // the runs of the tile's positions, one group each
        const int64_t g = (int64_t)(skey[pos] >> 32);
        const int64_t gs = gr.start[g], ge = gr.start[g + 1];
        const int64_t run_end = min(end, ge);
        if (gr.status[g] == ACTIVE) {
            const bool mine = live && p >= pos && p < run_end;
            double acc = 0.0;
            for (int64_t s0 = gs; s0 < ge; s0 += SRC) {
                const int cnt = (int)min((int64_t)SRC, ge - s0);
                __syncthreads();
                for (int k = lane; k < cnt; k += TILE) {
                    double4 v = mb.rec[s0 + k];
                    if (!mb.alive[s0 + k]) v.w = 0.0;          // a removed member: a zero-mass source
                    src[k] = v;
                }
                __syncthreads();
                if (mine) {
                    const int own = (int)min(p - s0, (int64_t)SRC);     // the target's own record, when it is in this tile
#pragma unroll 4
                    for (int k = 0; k < cnt; k++) {
                        const double4 s = src[k];
                        const double dx = r.x - s.x, dy = r.y - s.y, dz = r.z - s.z;
                        const double d2 = ((dx * dx + dy * dy) + dz * dz) + soft2;
                        const double rs = fast_rsqrt(d2);
                        const double sd = d2 > 0.0 ? d2 * rs : 0.0;     // s = sqrt(d2); 0 for coincident members, soft2 = 0
                        const double q = sd * inv_h;
                        const double term = (s.w * inv_h) * bound_phi(q, h * rs);
                        acc += (k == own) ? 0.0 : term;
                    }
                }
            }
            if (mine) {
                const double *G = gr.stat + g * NGS;
                const double dvx = mb.vx[p] - G[2], dvy = mb.vy[p] - G[3], dvz = mb.vz[p] - G[4];
                const double kin = 0.5 * ((dvx * dvx + dvy * dvy) + dvz * dvz);
                mb.phi[p] = acc;
                mb.e[p] = (thermal ? kin + mb.u[p] : kin) + acc;
            }
        }
        pos = run_end;
    }
}

// the most bound member: the smaller e, then the smaller id (order-free); a NaN e never wins
__device__ __forceinline__ void best_of(double &e, double &id, double e2, double id2) {
    if (e2 < e || (e2 == e && id2 < id)) { e = e2; id = id2; }
}

__global__ __launch_bounds__(BB) void bound_sums(Members mb, Groups gr, int64_t n_groups, int64_t n_pieces, int thermal, int round,
                                                 const int32_t *__restrict__ act, double *__restrict__ part) {
    if (act[round] == 0) return;
    const int64_t w = (int64_t)blockIdx.x * (BB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= n_pieces || w > gr.start[n_groups] / PIECE + n_groups) return;
    int64_t g, p0, p1;
    if (!piece_locate(gr.start, n_groups, w, g, p0, p1)) return;
    if (gr.status[g] != ACTIVE) return;
    const double *G = gr.stat + g * NGS;
    const double V[3] = {G[2], G[3], G[4]};
    double acc[NPB];
#pragma unroll
    for (int s = 0; s < NPB; s++) acc[s] = 0.0;
    acc[7] = INFINITY; acc[8] = INFINITY;
    for (int64_t p = p0 + lane; p < p1; p += WAVE) {
        if (!mb.alive[p]) continue;
        const double m = mb.m[p];
        const double4 r = mb.rec[p];
        const double dvx = mb.vx[p] - V[0], dvy = mb.vy[p] - V[1], dvz = mb.vz[p] - V[2];
        const double e = mb.e[p];
        acc[0] += (0.5 * m) * ((dvx * dvx + dvy * dvy) + dvz * dvz);
        acc[1] += m * mb.u[p];
        acc[2] += (0.5 * m) * mb.phi[p];
        acc[3] += m * r.x; acc[4] += m * r.y; acc[5] += m * r.z;
        if (e < 0.0) acc[6] += 1.0;
        best_of(acc[7], acc[8], e, (double)mb.id[p]);
    }
#pragma unroll
    for (int s = 0; s < 7; s++) acc[s] = wave_sum(acc[s]);
    for (int o = 32; o > 0; o >>= 1) best_of(acc[7], acc[8], __shfl_xor(acc[7], o, 64), __shfl_xor(acc[8], o, 64));
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NPB; s++) part[w * NPB + s] = acc[s];
    }
}

// a wavefront per active group: the row, and whether the group goes on (act[round + 1] counts those that do)
__global__ __launch_bounds__(BB) void bound_sums_final(Groups gr, Cfg cfg, int round, int32_t *__restrict__ act,
                                                       const double *__restrict__ part, double *__restrict__ table) {
    if (act[round] == 0) return;
    const int64_t g = (int64_t)blockIdx.x * (BB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= cfg.n_groups || gr.status[g] != ACTIVE) return;
    const int64_t len = (int64_t)gr.start[g + 1] - gr.start[g];
    const int64_t np = (len + PIECE - 1) / PIECE, base = piece_base(gr.start, g);
    double acc[NPB];
#pragma unroll
    for (int s = 0; s < NPB; s++) acc[s] = 0.0;
    acc[7] = INFINITY; acc[8] = INFINITY;
    for (int64_t k = lane; k < np; k += WAVE) {
        const double *q = part + (base + k) * NPB;
#pragma unroll
        for (int s = 0; s < 7; s++) acc[s] += q[s];
        best_of(acc[7], acc[8], q[7], q[8]);
    }
#pragma unroll
    for (int s = 0; s < 7; s++) acc[s] = wave_sum(acc[s]);
    for (int o = 32; o > 0; o >>= 1) best_of(acc[7], acc[8], __shfl_xor(acc[7], o, 64), __shfl_xor(acc[8], o, 64));
    if (lane != 0) return;
    const double *G = gr.stat + g * NGS;
    const double N = G[0], M = G[1], K = acc[0], U = acc[1], W = acc[2], neg = acc[6];
    const double KU = cfg.thermal ? K + U : K;
    const int R = gr.rounds[g];
    int st = ACTIVE;
    if (neg == N) st = 0;
    else if (R >= cfg.max_rounds) st = 1;
    else if (neg < (double)cfg.min_members) st = 2;
    if (table) {
        double *t = table + g * SPH_BOUND_NCOL;
        if (R == 0) {
            t[0] = N; t[1] = M; t[2] = K; t[3] = U; t[4] = W;
            t[5] = KU + W;
            t[6] = KU / fabs(W);
        }
        if (st == 2) {
            for (int c = 7; c < SPH_BOUND_NCOL; c++) t[c] = NAN;
            t[7] = 0.0; t[8] = 0.0; t[19] = 0.0; t[22] = -1.0;
        } else {
            const bool has = acc[7] < INFINITY;
            t[7] = N; t[8] = M;
            t[9] = acc[3] / M; t[10] = acc[4] / M; t[11] = acc[5] / M;
            t[12] = G[2]; t[13] = G[3]; t[14] = G[4];
            t[15] = K; t[16] = U; t[17] = W;
            t[18] = KU + W;
            t[19] = neg;
            t[22] = has ? acc[8] : -1.0;
            t[23] = has ? acc[7] : NAN;
        }
        t[20] = (double)R;
        t[21] = (double)(st == ACTIVE ? 1 : st);          // overwritten by the group's last evaluation
    }
    if (st == ACTIVE) {
        gr.rounds[g] = R + 1;
        atomicAdd(&act[round + 1], 1);
    } else {
        gr.status[g] = st;
    }
}

__global__ __launch_bounds__(BB) void bound_scatter(Members mb, Groups gr, const uint64_t *__restrict__ skey, int64_t n_slots,
                                                    int64_t n_groups, int64_t n, int32_t *__restrict__ labels,
                                                    double *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (p >= n_slots || p >= gr.start[n_groups]) return;
    const int64_t g = (int64_t)(skey[p] >> 32);
    const int32_t id = mb.id[p];
    const int st = gr.status[g];
    const double e = mb.e[p];
    if (labels) labels[id] = ((st == 0 || st == 1) && mb.alive[p] && e < 0.0) ? (int32_t)g : -1;
    if (out) { out[id] = e; out[n + id] = mb.phi[p]; }
}

// counts: members (-1: a member's h cannot be used), groups skipped, dissolved, stopped at max_rounds
__global__ __launch_bounds__(BB) void bound_counts(Groups gr, int64_t n_groups, const int32_t *__restrict__ bad,
                                                   unsigned long long *__restrict__ counts) {
    const int64_t g = (int64_t)blockIdx.x * BB + threadIdx.x;
    if (g == 0) counts[0] = *bad ? ~0ull : (unsigned long long)gr.start[n_groups];
    const int st = (g < n_groups && !*bad) ? gr.status[g] : 0;
    const unsigned long long b3 = __ballot(st == 3), b2 = __ballot(st == 2), b1 = __ballot(st == 1);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (b3) atomicAdd(&counts[1], (unsigned long long)__popcll(b3));
        if (b2) atomicAdd(&counts[2], (unsigned long long)__popcll(b2));
        if (b1) atomicAdd(&counts[3], (unsigned long long)__popcll(b1));
    }
}

}  // namespace

int bound_run(sph_ctx *c, const sph_bound_desc *d, const int32_t *labels, int64_t n_labels, int64_t n_groups,
              int32_t *bound_labels, double *out, int64_t n_out, double *table, int64_t *counts, bool host) {
    const char *who = "sph_bound";
    if (!d) return arg_error(c, who, "null descriptor");
    if (!labels) return arg_error(c, who, "null labels");
    if (!bound_labels && !out && !table && !counts) return arg_error(c, who, "no output");
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return arg_error(c, who, "reserved must be 0");
    if (d->flags & ~SPH_BOUND_THERMAL) return arg_error(c, who, "unknown flags");
    if (n_labels != c->n) return arg_error(c, who, "n_labels != sph_count");
    if (out && n_out != 2 * c->n) return arg_error(c, who, "n_out != 2 sph_count");
    if (n_groups < 0 || n_groups > 0x7fffffffLL) return arg_error(c, who, "n_groups must be 0 .. 2^31 - 1");
    if (d->min_members < 1) return arg_error(c, who, "min_members must be >= 1");
    if (d->max_members < 1) return arg_error(c, who, "max_members must be >= 1");
    if (d->max_rounds < 0) return arg_error(c, who, "max_rounds must be >= 0");
    if (std::isnan(d->h) || d->h < 0.0) return arg_error(c, who, "h must be >= 0");
    if (std::isnan(d->soft2) || d->soft2 < 0.0) return arg_error(c, who, "soft2 must be >= 0");
    const bool own_h = !(d->h > 0.0);
    if (own_h && !c->variable && !(c->p.h > 0.0 && std::isfinite(c->p.h))) {
        c->err = "sph_bound: params.h <= 0 on a fixed-h context (give desc.h > 0)";
        return SPH_ERR_STATE;
    }

    hipStream_t st = c->stream;
    const int64_t n = c->n, no = c->n_owned;
    const int64_t ns = c->cap > 0 ? c->n_slots : 0;
    const int64_t ng = n_groups;
    if (ns == 0 || no == 0 || ng == 0) {            // no member: the defaults, rows of empty groups, zero counts
        if (host) {
            if (bound_labels) std::fill(bound_labels, bound_labels + n, -1);
            if (out) std::fill(out, out + 2 * n, (double)NAN);
            if (table)
                for (int64_t g = 0; g < ng; g++) {
                    double *t = table + g * SPH_BOUND_NCOL;
                    std::fill(t, t + SPH_BOUND_NCOL, (double)NAN);
                    t[0] = 0.0; t[7] = 0.0; t[8] = 0.0; t[19] = 0.0; t[20] = 0.0; t[21] = 2.0; t[22] = -1.0;
                }
            if (counts) { counts[0] = 0; counts[1] = 0; counts[2] = ng; counts[3] = 0; }
            return SPH_OK;
        }
        if (n > 0 && (bound_labels || out))
            bound_fill<<<dim3(blocks(n, BB)), dim3(BB), 0, st>>>(n, bound_labels, out);
        SPH_HIP(hipGetLastError());
        if (ng > 0 && (table || counts)) {
            // the rows and the count of the empty groups come from the general path below on an empty member list; with
            // no slot at all there is no list to search, so the groups are initialised from a zeroed start table
            int32_t *start, *status, *rounds, *bad, *act;
            auto layout = [&](Carve cv) {
                start = cv.take<int32_t>(ng + 1);
                status = cv.take<int32_t>(ng);
                rounds = cv.take<int32_t>(ng);
                bad = cv.take<int32_t>(1);
                act = cv.take<int32_t>(1);
                return cv.bytes;
            };
            char *buf = nullptr;
            SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
            layout(Carve{buf});
            SPH_HIP(hipMemsetAsync(start, 0, sizeof(int32_t) * (size_t)(ng + 1), st));
            SPH_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
            SPH_HIP(hipMemsetAsync(act, 0, sizeof(int32_t), st));
            Cfg cfg{};
            cfg.n_groups = ng; cfg.min_members = d->min_members; cfg.max_members = d->max_members;
            Groups gr{start, status, rounds, nullptr};
            bound_init<<<dim3(blocks(ng, BB)), dim3(BB), 0, st>>>(cfg, gr, bad, table, act);
            if (counts) {
                SPH_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st));
                bound_counts<<<dim3(blocks(ng, BB)), dim3(BB), 0, st>>>(gr, ng, bad, reinterpret_cast<unsigned long long *>(counts));
            }
            SPH_HIP(hipGetLastError());
        } else if (counts) {
            SPH_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), st));
        }
        return SPH_OK;
    }

    // a round removes at least one member of every group that goes on: no group sees more than N_0 - 1 removals
    const int64_t most = std::min<int64_t>(std::min<int64_t>(no, d->max_members) - 1, d->max_rounds);
    const int n_rounds = (int)std::max<int64_t>(most, 0) + 1;              // evaluations enqueued at most
    const int64_t n_pieces = ns / PIECE + ng + 1;
    const int64_t n_tiles = (ns + TILE - 1) / TILE;
    size_t sort_bytes = 0;
    SPH_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)ns, 0u, 64u, st));
    uint64_t *keys, *keys_alt;
    uint32_t *vals, *vals_alt;
    char *sort_tmp;
    Members mb{};
    Groups gr{};
    int32_t *bad, *act, *n_list, *list, *h_labels_in, *h_labels;
    double *part, *h_out, *h_table;
    unsigned long long *cnt;
    auto layout = [&](Carve cv) {
        keys = cv.take<uint64_t>(ns);
        keys_alt = cv.take<uint64_t>(ns);
        vals = cv.take<uint32_t>(ns);
        vals_alt = cv.take<uint32_t>(ns);
        sort_tmp = cv.take<char>(sort_bytes);
        mb.rec = cv.take<double4>(ns);
        mb.h = cv.take<double>(ns); mb.vx = cv.take<double>(ns); mb.vy = cv.take<double>(ns); mb.vz = cv.take<double>(ns);
        mb.u = cv.take<double>(ns); mb.m = cv.take<double>(ns); mb.e = cv.take<double>(ns); mb.phi = cv.take<double>(ns);
        mb.id = cv.take<int32_t>(ns);
        mb.alive = cv.take<uint8_t>(ns);
        gr.start = cv.take<int32_t>(ng + 1);
        gr.status = cv.take<int32_t>(ng);
        gr.rounds = cv.take<int32_t>(ng);
        gr.stat = cv.take<double>(NGS * (size_t)ng);
        part = cv.take<double>(NPB * (size_t)n_pieces);
        list = cv.take<int32_t>(n_tiles);
        bad = cv.take<int32_t>(1);
        act = cv.take<int32_t>((size_t)n_rounds + 1);
        n_list = cv.take<int32_t>((size_t)n_rounds);
        cnt = cv.take<unsigned long long>(4);
        h_labels_in = cv.take<int32_t>(host ? n : 0);                            // the host form's device copies
        h_labels = cv.take<int32_t>(host && bound_labels ? n : 0);
        h_out = cv.take<double>(host && out ? 2 * (size_t)n : 0);
        h_table = cv.take<double>(host && table ? SPH_BOUND_NCOL * (size_t)ng : 0);
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    if (host) SPH_TRY(analysis_pinned(c));
    const int32_t *d_in = labels;
    if (host) {
        SPH_HIP(hipMemcpyAsync(h_labels_in, labels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        d_in = h_labels_in;
    }
    int32_t *d_labels = bound_labels ? (host ? h_labels : bound_labels) : nullptr;
    double *d_out = out ? (host ? h_out : out) : nullptr;
    double *d_table = table ? (host ? h_table : table) : nullptr;

    Cfg cfg{};
    cfg.soft2 = d->soft2;
    cfg.fixed_h = own_h ? c->p.h : d->h;
    cfg.hf = own_h && c->variable ? c->f[SPH_F_H] : nullptr;
    cfg.G = c->p.G;
    cfg.n_owned = no; cfg.n_groups = ng; cfg.min_members = d->min_members; cfg.max_members = d->max_members;
    cfg.max_rounds = d->max_rounds;
    cfg.thermal = (d->flags & SPH_BOUND_THERMAL) ? 1 : 0;
    Fields f{c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], c->f[SPH_F_VX], c->f[SPH_F_VY], c->f[SPH_F_VZ], c->f[SPH_F_U],
             c->f[SPH_F_M], c->orig};

    SPH_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    SPH_HIP(hipMemsetAsync(act, 0, sizeof(int32_t) * ((size_t)n_rounds + 1), st));
    SPH_HIP(hipMemsetAsync(n_list, 0, sizeof(int32_t) * (size_t)n_rounds, st));
    SPH_HIP(hipMemsetAsync(cnt, 0, 4 * sizeof(unsigned long long), st));
    if (d_labels || d_out) bound_fill<<<dim3(blocks(n, BB)), dim3(BB), 0, st>>>(n, d_labels, d_out);
    bound_keys<<<dim3(blocks(ns, BB)), dim3(BB), 0, st>>>(f.x, f.y, f.z, c->orig, ns, no, ng, d_in, keys, vals);
    SPH_HIP(hipGetLastError());
    size_t tmp = sort_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, keys, keys_alt, vals, vals_alt, (size_t)ns, 0u, 64u, st));
    bound_starts<<<dim3(blocks(ng + 1, BB)), dim3(BB), 0, st>>>(keys_alt, ns, ng, gr.start);
    bound_gather<<<dim3(blocks(ns, BB)), dim3(BB), 0, st>>>(f, cfg, vals_alt, gr.start, ns, mb, bad);
    bound_init<<<dim3(blocks(ng, BB)), dim3(BB), 0, st>>>(cfg, gr, bad, d_table, act);
    SPH_HIP(hipGetLastError());

    const int wpb = BB / WAVE;
    for (int r = 0; r < n_rounds; r++) {
        bound_mom<<<dim3(blocks(n_pieces, wpb)), dim3(BB), 0, st>>>(mb, gr, ng, n_pieces, r, act, part);
        bound_mom_final<<<dim3(blocks(ng, wpb)), dim3(BB), 0, st>>>(gr, ng, r, act, part);
        bound_plan<<<dim3(blocks(n_tiles, BB)), dim3(BB), 0, st>>>(mb, gr, keys_alt, ng, n_tiles, r, act, list, n_list);
        bound_pairs<<<dim3((unsigned)n_tiles), dim3(TILE), 0, st>>>(mb, gr, keys_alt, ng, cfg.soft2, cfg.thermal, r, act, list,
                                                                    n_list);
        bound_sums<<<dim3(blocks(n_pieces, wpb)), dim3(BB), 0, st>>>(mb, gr, ng, n_pieces, cfg.thermal, r, act, part);
        bound_sums_final<<<dim3(blocks(ng, wpb)), dim3(BB), 0, st>>>(gr, cfg, r, act, part, d_table);
        SPH_HIP(hipGetLastError());
        if (host && r + 1 < n_rounds) {              // the host form stops enqueueing once every group has finished
            SPH_HIP(hipMemcpyAsync(c->rnd_pinned, act + r + 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            SPH_HIP(hipStreamSynchronize(st));
            int32_t going = 0;
            std::memcpy(&going, c->rnd_pinned, sizeof(int32_t));
            if (going == 0) break;
        }
    }
    if (d_labels || d_out)
        bound_scatter<<<dim3(blocks(ns, BB)), dim3(BB), 0, st>>>(mb, gr, keys_alt, ns, ng, n, d_labels, d_out);
    bound_counts<<<dim3(blocks(ng, BB)), dim3(BB), 0, st>>>(gr, ng, bad, cnt);
    SPH_HIP(hipGetLastError());
    if (!host) {
        if (counts) SPH_HIP(hipMemcpyAsync(counts, cnt, 4 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        return SPH_OK;
    }
    // host form: the counts first (a bad h writes nothing), then the copies out
    SPH_HIP(hipMemcpyAsync(c->rnd_pinned, cnt, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    int64_t cc[4];
    std::memcpy(cc, c->rnd_pinned, sizeof(cc));
    if (cc[0] < 0) {
        c->err = "sph_bound: a member has h <= 0 or a non-finite h";
        return SPH_ERR_STATE;
    }
    if (bound_labels && n > 0) SPH_HIP(hipMemcpyAsync(bound_labels, d_labels, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (out && n > 0) SPH_HIP(hipMemcpyAsync(out, d_out, 2 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (table) SPH_HIP(hipMemcpyAsync(table, d_table, SPH_BOUND_NCOL * (size_t)ng * sizeof(double), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    if (counts) std::memcpy(counts, cc, sizeof(cc));
    return SPH_OK;
}

}  // namespace sph
