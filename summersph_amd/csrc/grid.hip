// grid.hip -- the neighbour index: uniform cell grid + radix-sorted particle order.
//
// Replaces the reference's pointer octree (create_tree / build_tree,
// /root/reference/SUMMER_SPH.f90:795-816,149-246) for the fixed-h path.  Only the octree's
// SEMANTICS are kept: for fixed h the tree walk visits exactly {j : |x_i - x_j| <= 2h}
// (SURVEY.md 3.2), which a grid of edge 2h and a 27-cell stencil also covers.
//
// Pipeline per rebuild (all on ctx->stream):
//   bbox_partial/bbox_final  -> bounding box (one small read-back: the host sizes the grid)
//   cell_keys                -> 32-bit key per particle, axis with fewest cells fastest
//   rocprim radix sort       -> stable (key, slot) sort on only as many bits as the grid needs
//   cell_table               -> cell_start[c] = first sorted slot with key >= c
//   reorder                  -> gathers the 9 state arrays + ids into sorted order and writes
//                               the 32-byte density gather record {x,y,z,m}
// Inside sph_run / sph_step the steady state of the plain fixed-h path (dense table, counting sort, the box of the previous
// build) folds four of these launches into their neighbours: the opening kick + drift writes keys, histogram and box partials
// (kick_drift_keys), the box is finished by one workgroup more of cell_scatter, reorder_ranked takes the rank within the cell
// itself; a context of one rank without ghosts leaves inv to ensure_inv.  Same keys, table, box, permutation: same bits.
// Hashed grids (boxes too sparse for a dense table, see grid_rebuild): 64-bit keys, a radix sort over the key bits in use,
// run heads -> scan -> the occupied cells (ukey, ustart), and a hash table over them (sph_internal.hpp HashView).
#include <cstdlib>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cmath>
#include <utility>

#include "pair_common.hpp"
#include "integ_common.hpp"

namespace sph {

namespace {

constexpr int BB_BLOCK = 256;
constexpr int BB_MAX_BLOCKS = 1024;

__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// partial[b*6 + {0..2}] = min x,y,z ; {3..5} = max x,y,z over block b's grid-stride share
// mode 0: every slot except replaced ghosts (slot < dead_below with original id >= n_owned); mode 1: owned only
__global__ __launch_bounds__(BB_BLOCK) void bbox_partial(const double *__restrict__ x, const double *__restrict__ y,
                                                         const double *__restrict__ z, int64_t n,
                                                         double *__restrict__ partial, int32_t *__restrict__ flags,
                                                         const int32_t *__restrict__ orig, int32_t n_owned,
                                                         int64_t dead_below, int owned_only) {
    __shared__ double sm[6][BB_BLOCK / WAVE];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * BB_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BB_BLOCK) {
        if ((owned_only || i < dead_below) && orig[i] >= n_owned) continue;
        double v[3] = {x[i], y[i], z[i]};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            bad |= !isfinite(v[a]);
            lo[a] = fmin(lo[a], v[a]);
            hi[a] = fmax(hi[a], v[a]);
        }
    }
    if (bad) flags[0] = 1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double mn = wave_min(lo[a]), mx = wave_max(hi[a]);
        if (lane == 0) { sm[a][wv] = mn; sm[3 + a][wv] = mx; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double r = sm[threadIdx.x][0];
        for (int k = 1; k < BB_BLOCK / WAVE; k++)
            r = threadIdx.x < 3 ? fmin(r, sm[threadIdx.x][k]) : fmax(r, sm[threadIdx.x][k]);
        partial[(int64_t)blockIdx.x * 6 + threadIdx.x] = r;
    }
}

// 6 waves, one per bbox component; lanes stride over the per-block partials.  host_slot (pinned host memory, mapped into the
// device's address space) gets the box and the non-finite flag directly: a separate device-to-host copy of 52 bytes costs
// a copy kernel of ~16 us on the stream (two of them per grid build were 3 % of the bench step)
__device__ __forceinline__ void bbox_final_comp(int comp, int lane, const double *__restrict__ partial, int nblocks,
                                                double *__restrict__ out, double *__restrict__ host_slot, int32_t *__restrict__ flags) {
    double r = comp < 3 ? INFINITY : -INFINITY;
    for (int b = lane; b < nblocks; b += 64) {
        const double v = partial[b * 6 + comp];
        r = comp < 3 ? fmin(r, v) : fmax(r, v);
    }
    r = comp < 3 ? wave_min(r) : wave_max(r);
    if (lane == 0) {
        out[comp] = r;
        if (host_slot) {
            host_slot[comp] = r;
            if (comp == 0) { *reinterpret_cast<int32_t *>(host_slot + 6) = flags[0]; flags[0] = 0; }     // ... and cleared for the next build
        }
    }
}

__global__ __launch_bounds__(384) void bbox_final(const double *__restrict__ partial, int nblocks, double *__restrict__ out,
                                                  double *__restrict__ host_slot = nullptr, int32_t *__restrict__ flags = nullptr) {
    bbox_final_comp(threadIdx.x >> 6, threadIdx.x & 63, partial, nblocks, out, host_slot, flags);
}

// count, sum and sum of squares per axis of the live particles inside box (lo, hi): partial[b*7 + ...].  For the trimmed
// grid box of very sparse domains (grid_rebuild); two stages with a fixed order, like the bounding box.
struct Box6 { double lo[3], hi[3]; };
__global__ __launch_bounds__(BB_BLOCK) void moment_partial(const double *__restrict__ x, const double *__restrict__ y,
                                                           const double *__restrict__ z, int64_t n, Box6 box,
                                                           double *__restrict__ partial, const int32_t *__restrict__ orig,
                                                           int32_t n_owned, int64_t dead_below) {
    __shared__ double sm[7][BB_BLOCK / WAVE];
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * BB_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BB_BLOCK) {
        if (i < dead_below && orig[i] >= n_owned) continue;
        const double v[3] = {x[i], y[i], z[i]};
        const bool in = v[0] >= box.lo[0] && v[0] <= box.hi[0] && v[1] >= box.lo[1] && v[1] <= box.hi[1] && v[2] >= box.lo[2] && v[2] <= box.hi[2];
        if (!in) continue;
        acc[0] += 1.0;
#pragma unroll
        for (int a = 0; a < 3; a++) { acc[1 + a] += v[a]; acc[4 + a] += v[a] * v[a]; }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        double r = acc[k];
        for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o, 64);
        if (lane == 0) sm[k][wv] = r;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        double r = 0.0;
        for (int k = 0; k < BB_BLOCK / WAVE; k++) r += sm[threadIdx.x][k];
        partial[(int64_t)blockIdx.x * 7 + threadIdx.x] = r;
    }
}

__global__ __launch_bounds__(448) void moment_final(const double *__restrict__ partial, int nblocks, double *__restrict__ out) {
    const int comp = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double r = 0.0;
    for (int b = lane; b < nblocks; b += 64) r += partial[b * 7 + comp];
    for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o, 64);
    if (lane == 0) out[comp] = r;
}

__device__ __forceinline__ uint32_t cell_key(const GridDesc &g, double px, double py, double pz, int cc[3]) {
    const double p[3] = {px, py, pz};
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        // clamped as a double BEFORE the cast: a particle far outside the (stale or trimmed) box, or a NaN that is reported a
        // build late, must not reach an out-of-range float -> int conversion (undefined in C++); fmax drops a NaN -> cell 0
        c[a] = (int)fmin(fmax((p[a] - g.org[a]) * g.inv_edge, 0.0), (double)(g.dim[a] - 1));
    }
    cc[0] = c[g.s[0]]; cc[1] = c[g.s[1]]; cc[2] = c[g.s[2]];
    return ((uint32_t)cc[2] * (uint32_t)g.dim[g.s[1]] + (uint32_t)cc[1]) * (uint32_t)g.dim[g.s[0]] + (uint32_t)cc[0];
}

// replaced ghosts (slot < dead_below, original id >= n_owned) get the key ncells: they sort behind every cell
__global__ __launch_bounds__(256) void cell_keys(GridDesc g, const double *__restrict__ x, const double *__restrict__ y,
                                                 const double *__restrict__ z, int64_t n, uint32_t *__restrict__ keys,
                                                 uint32_t *__restrict__ vals, const int32_t *__restrict__ orig,
                                                 int32_t n_owned, int64_t dead_below) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int cc[3];
    const bool dead = i < dead_below && orig[i] >= n_owned;
    keys[i] = dead ? (uint32_t)g.ncells : cell_key(g, x[i], y[i], z[i], cc);
    vals[i] = (uint32_t)i;
}

// ---- counting sort by cell (the default; the radix sort below remains for grids with far more cells than particles) ----
// The sorted order wanted is that of a STABLE sort of (cell key, slot): cells ascending, within a cell the slots in their
// previous order.  keys + histogram -> exclusive scan = cell table -> scatter with a per-cell cursor (arrival order, not
// reproducible) -> every entry is moved to its rank among the entries of its cell (reproducible again).
// ~70 us at 1e6 particles against ~165 us for rocprim's 21-launch merge sort of the same pairs + the table search.
// The slots are nearly sorted already (last step's order), so the lanes of a wave hold a few runs of equal keys: one atomic
// per run instead of one per lane (42 -> ~10 us for the histogram, 60 -> ~15 us for the scatter at 1e6 particles).
// Returns this lane's offset within its run and, for the run's first lane, the run length (0 for the others).
__device__ __forceinline__ int run_of_equal_keys(uint32_t k, bool valid, int &run_len, int &head_lane) {
    const int lane = threadIdx.x & 63;
    const uint32_t prev = (uint32_t)__shfl_up((int)k, 1, 64);
    const bool pvalid = __shfl_up(valid ? 1 : 0, 1, 64) != 0;
    const bool head = valid && (lane == 0 || !pvalid || prev != k);
    // a run ends where the next head starts or where the valid lanes end
    const uint64_t heads = __ballot(head), ends = heads | ~__ballot(valid);
    const uint64_t below = heads & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));          // heads at or below this lane
    head_lane = below ? 63 - __clzll((long long)below) : lane;
    const uint64_t above = lane == 63 ? 0ull : (ends >> (lane + 1));                           // first boundary above this lane
    const int next = above ? lane + 1 + (__ffsll((long long)above) - 1) : 64;
    run_len = head ? next - lane : 0;
    return lane - head_lane;
}

__global__ __launch_bounds__(256) void cell_keys_count(GridDesc g, const double *__restrict__ x, const double *__restrict__ y,
                                                       const double *__restrict__ z, int64_t n, uint32_t *__restrict__ keys,
                                                       int32_t *__restrict__ count, const int32_t *__restrict__ orig,
                                                       int32_t n_owned, int64_t dead_below) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n;
    uint32_t k = 0;
    if (valid) {
        int cc[3];
        const bool dead = i < dead_below && orig[i] >= n_owned;
        k = dead ? (uint32_t)g.ncells : cell_key(g, x[i], y[i], z[i], cc);
        keys[i] = k;
    }
    int run_len, head_lane;
    run_of_equal_keys(k, valid, run_len, head_lane);
    if (run_len > 0) atomicAdd(&count[k], run_len);
}

// The opening kick + drift of a fixed-h step (integrate.hip: kick_drift_kernel, the same expressions and bits) which goes on
// with the new position while it is in registers: the work of cell_keys_count (key, histogram) and of bbox_partial (mode 0, no
// replaced ghosts).  Minimum, maximum and integer counts do not depend on the order: keys, table, box and flag are those of
// the separate launches.  Blocks stride over the particles beyond EARLY_MAX_BLOCKS * 256 of them.
struct KickDriftArgs {
    double *x, *y, *z, *vx, *vy, *vz, *u, *alpha;
    const double *ax, *ay, *az, *du, *dalpha;
};

__global__ __launch_bounds__(256) void kick_drift_keys(KickDriftArgs a, GridDesc g, int64_t n, const double *__restrict__ dt_ptr,
                                                       double *__restrict__ sink, int ns, uint32_t *__restrict__ keys,
                                                       int32_t *__restrict__ count, double *__restrict__ partial,
                                                       int32_t *__restrict__ flags) {
    __shared__ double sm[6][256 / WAVE];
    const double dt = dt_ptr[0];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < n;
        uint32_t k = 0;
        if (valid) {
            const double vx = kick_half(a.vx[i], a.ax[i], dt), vy = kick_half(a.vy[i], a.ay[i], dt), vz = kick_half(a.vz[i], a.az[i], dt);
            a.vx[i] = vx; a.vy[i] = vy; a.vz[i] = vz;
            a.u[i] = kick_half(a.u[i], a.du[i], dt);
            a.alpha[i] = kick_alpha(a.alpha[i], a.dalpha[i], dt);
            const double v[3] = {drift_pos(a.x[i], vx, dt), drift_pos(a.y[i], vy, dt), drift_pos(a.z[i], vz, dt)};
            a.x[i] = v[0]; a.y[i] = v[1]; a.z[i] = v[2];
#pragma unroll
            for (int d = 0; d < 3; d++) {
                bad |= !isfinite(v[d]);
                lo[d] = fmin(lo[d], v[d]);
                hi[d] = fmax(hi[d], v[d]);
            }
            int cc[3];
            k = cell_key(g, v[0], v[1], v[2], cc);
            keys[i] = k;
        }
        int run_len, head_lane;
        run_of_equal_keys(k, valid, run_len, head_lane);
        if (run_len > 0) atomicAdd(&count[k], run_len);
    }
    if (bad) flags[0] = 1;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double mn = wave_min(lo[d]), mx = wave_max(hi[d]);
        if (lane == 0) { sm[d][wv] = mn; sm[3 + d][wv] = mx; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double r = sm[threadIdx.x][0];
        for (int w = 1; w < 256 / WAVE; w++)
            r = threadIdx.x < 3 ? fmin(r, sm[threadIdx.x][w]) : fmax(r, sm[threadIdx.x][w]);
        partial[(int64_t)blockIdx.x * 6 + threadIdx.x] = r;
    }
    if (blockIdx.x == 0 && threadIdx.x < ns) {
        const int s = threadIdx.x;
        for (int d = 0; d < 3; d++) {
            const double v = sink[(3 + d) * MAX_SINKS + s] + 0.5 * sink[(7 + d) * MAX_SINKS + s] * dt;
            sink[(3 + d) * MAX_SINKS + s] = v;
            sink[d * MAX_SINKS + s] = sink[d * MAX_SINKS + s] + v * dt;
        }
    }
}

// the box partials of kick_drift_keys: reduced by one workgroup more of cell_scatter, a few launches later, instead of
// by a launch of their own (no fence: the partials come from an earlier kernel of the stream)
struct BoxFinal {
    const double *partial;
    int nblocks;
    double *out, *host_slot;
    int32_t *flags;
};

// 256 threads stride over the blocks' partials (six contiguous doubles each: three 16-byte loads in flight per trip), then
// the waves and the workgroup; minimum and maximum do not depend on the order
__device__ __forceinline__ void bbox_final_block(const BoxFinal &bf) {
    __shared__ double sm[6][256 / WAVE];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < bf.nblocks; b += 256) {
        const double2 *q = reinterpret_cast<const double2 *>(bf.partial + (size_t)b * 6);
        const double2 v0 = q[0], v1 = q[1], v2 = q[2];
        lo[0] = fmin(lo[0], v0.x); lo[1] = fmin(lo[1], v0.y); lo[2] = fmin(lo[2], v1.x);
        hi[0] = fmax(hi[0], v1.y); hi[1] = fmax(hi[1], v2.x); hi[2] = fmax(hi[2], v2.y);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double mn = wave_min(lo[d]), mx = wave_max(hi[d]);
        if (lane == 0) { sm[d][wv] = mn; sm[3 + d][wv] = mx; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double r = sm[threadIdx.x][0];
        for (int w = 1; w < 256 / WAVE; w++)
            r = threadIdx.x < 3 ? fmin(r, sm[threadIdx.x][w]) : fmax(r, sm[threadIdx.x][w]);
        bf.out[threadIdx.x] = r;
        bf.host_slot[threadIdx.x] = r;
        if (threadIdx.x == 0) { *reinterpret_cast<int32_t *>(bf.host_slot + 6) = bf.flags[0]; bf.flags[0] = 0; }     // as bbox_final
    }
}

template <bool BOX>
__global__ __launch_bounds__(256) void cell_scatter(const uint32_t *__restrict__ keys, int64_t n, const int32_t *__restrict__ cell_start,
                                                    int32_t *__restrict__ fill, uint32_t *__restrict__ slots, BoxFinal bf) {
    if (BOX && blockIdx.x == gridDim.x - 1) {
        bbox_final_block(bf);
        return;
    }
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n;
    const uint32_t k = valid ? keys[i] : 0u;
    int run_len, head_lane;
    const int off = run_of_equal_keys(k, valid, run_len, head_lane);
    int base = 0;
    if (run_len > 0) base = cell_start[k] + atomicAdd(&fill[k], run_len);
    base = __shfl(base, head_lane, 64);
    if (valid) slots[base + off] = (uint32_t)i;
}

// p < n_live: entry slots[p] of cell k goes to cell_start[k] + (number of entries of the cell that are smaller)
__global__ __launch_bounds__(256) void cell_rank(const uint32_t *__restrict__ keys, int64_t n_live, const int32_t *__restrict__ cell_start,
                                                 const uint32_t *__restrict__ slots, uint32_t *__restrict__ sorted) {
    int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_live) return;
    const uint32_t v = slots[p];
    const uint32_t k = keys[v];
    const int s = cell_start[k], e = cell_start[k + 1];
    int rank = 0;
    for (int q = s; q < e; q++) rank += slots[q] < v ? 1 : 0;
    sorted[s + rank] = v;
}

// cell_start[c] = lower_bound(sorted keys, c), c in [0, ncells]
__global__ __launch_bounds__(256) void cell_table(const uint32_t *__restrict__ keys, int64_t n, int64_t ncells,
                                                  int32_t *__restrict__ cell_start) {
    int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c > ncells) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < c) lo = mid + 1; else hi = mid;
    }
    cell_start[c] = (int32_t)lo;
}

// ---- hashed cell table --------------------------------------------------------------------------
// key = c2 << sh2 | c1 << sh1 | c0 (permuted axes): the dense key's order.  Replaced ghosts get ~0 and sort behind every cell.
__global__ __launch_bounds__(256) void hash_keys(GridDesc g, int32_t sh1, int32_t sh2, const double *__restrict__ x,
                                                 const double *__restrict__ y, const double *__restrict__ z, int64_t n,
                                                 uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                 const int32_t *__restrict__ orig, int32_t n_owned, int64_t dead_below) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool dead = i < dead_below && orig[i] >= n_owned;
    uint64_t k = ~0ull;
    if (!dead) {
        int cc[3];
        cell_coords(g, x[i], y[i], z[i], cc);
        k = ((uint64_t)cc[2] << sh2) | ((uint64_t)cc[1] << sh1) | (uint64_t)cc[0];
    }
    keys[i] = k;
    vals[i] = (uint32_t)i;
}

// head[p] = 1 where a run of equal keys starts (p < n live entries of the sorted keys)
__global__ __launch_bounds__(256) void hash_heads(const uint64_t *__restrict__ keys, int64_t n, int32_t *__restrict__ head) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) head[p] = (p == 0 || keys[p] != keys[p - 1]) ? 1 : 0;
}

// uidx = inclusive scan of the heads: ukey[u] / ustart[u] of the u-th occupied cell, ustart[m] = n, *m_out = m
__global__ __launch_bounds__(256) void hash_compact(const uint64_t *__restrict__ keys, const int32_t *__restrict__ uidx, int64_t n,
                                                   uint64_t *__restrict__ ukey, int32_t *__restrict__ ustart, int32_t *__restrict__ m_out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint64_t k = keys[p];
    if (p == 0 || k != keys[p - 1]) { ukey[uidx[p] - 1] = k; ustart[uidx[p] - 1] = (int32_t)p; }
    if (p == n - 1) { const int32_t m = uidx[p]; *m_out = m; ustart[m] = (int32_t)n; ukey[m] = ~0ull; }
}

__device__ __forceinline__ void hash_put(HashEnt *__restrict__ tab, uint64_t mask, uint64_t key, int32_t idx, int32_t start) {
    for (uint64_t s = hash_mix(key) & mask;; s = (s + 1) & mask) {
        const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(&tab[s].key), ~0ull, (unsigned long long)key);
        // a key inserted twice (k + 1 of one cell = the next occupied cell) carries the same values both times
        if (prev == ~0ull || prev == key) { tab[s].idx = idx; tab[s].start = start; return; }
    }
}

// every occupied cell u: key -> {u, ustart[u]} and key + 1 -> {u + 1, ustart[u + 1]} (the lower bound just behind the cell)
__global__ __launch_bounds__(256) void hash_insert(const uint64_t *__restrict__ ukey, const int32_t *__restrict__ ustart,
                                                   const int32_t *__restrict__ m_ptr, HashEnt *__restrict__ tab, uint64_t mask) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= *m_ptr) return;
    const uint64_t k = ukey[u];
    hash_put(tab, mask, k, (int32_t)u, ustart[u]);
    hash_put(tab, mask, k + 1, (int32_t)u + 1, ustart[u + 1]);
}

struct ReorderArgs {
    const double *src[10];
    double *dst[10];
    int nf;            // 9 state fields, 10 with the smoothing length (variable-h path)
    double *prec;      // variable-h: {x,y,z,h} gather record, else nullptr
};

__global__ __launch_bounds__(256) void reorder(ReorderArgs a, const uint32_t *__restrict__ perm,
                                               const int32_t *__restrict__ orig_in, int32_t *__restrict__ orig_out,
                                               int32_t *__restrict__ inv, double *__restrict__ drec, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = perm[i];
    double v[10];
#pragma unroll
    for (int k = 0; k < 10; k++) v[k] = k < a.nf ? a.src[k][s] : 0.0;
#pragma unroll
    for (int k = 0; k < 10; k++)
        if (k < a.nf) a.dst[k][i] = v[k];
    if (a.prec) reinterpret_cast<double4 *>(a.prec)[i] = make_double4(v[SPH_F_X], v[SPH_F_Y], v[SPH_F_Z], v[9]);
    const int32_t id = orig_in[s];
    orig_out[i] = id;
    if (inv) inv[id] = (int32_t)i;        // original id -> sorted slot (nullptr: rebuilt from orig when somebody asks, ensure_inv)
    double4 r = make_double4(v[SPH_F_X], v[SPH_F_Y], v[SPH_F_Z], v[SPH_F_M]);
    reinterpret_cast<double4 *>(drec)[i] = r;
}

// cell_rank and reorder in one pass for the fixed-h state (nine fields): entry slots[p] of cell k moves straight to
// cell_start[k] + its rank among the cell's entries -- the permutation cell_rank writes for reorder to read back, so the same
// bits; the stores of a wave scatter within its few cells, i.e. within the lines the wave fills anyway
__global__ __launch_bounds__(256) void reorder_ranked(ReorderArgs a, const uint32_t *__restrict__ keys, const int32_t *__restrict__ cell_start,
                                                      const uint32_t *__restrict__ slots, const int32_t *__restrict__ orig_in,
                                                      int32_t *__restrict__ orig_out, int32_t *__restrict__ inv,
                                                      double *__restrict__ drec, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t s = slots[p];
    const uint32_t k = keys[s];
    const int cs = cell_start[k], ce = cell_start[k + 1];
    double v[9];
#pragma unroll
    for (int f = 0; f < 9; f++) v[f] = a.src[f][s];
    const int32_t id = orig_in[s];
    int rank = 0;
    for (int q = cs; q < ce; q++) rank += slots[q] < s ? 1 : 0;
    const int64_t i = cs + rank;
#pragma unroll
    for (int f = 0; f < 9; f++) a.dst[f][i] = v[f];
    orig_out[i] = id;
    if (inv) inv[id] = (int32_t)i;
    reinterpret_cast<double4 *>(drec)[i] = make_double4(v[SPH_F_X], v[SPH_F_Y], v[SPH_F_Z], v[SPH_F_M]);
}

__global__ __launch_bounds__(256) void inv_from_orig(const int32_t *__restrict__ orig, int32_t *__restrict__ inv, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) inv[orig[i]] = (int32_t)i;
}

__global__ __launch_bounds__(256) void iota_kernel(int32_t *p, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void unpermute(const double *__restrict__ src, const int32_t *__restrict__ orig,
                                                 double *__restrict__ dst, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[orig[i]] = src[i];
}

__global__ __launch_bounds__(256) void fill_kernel(double *p, double v, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// dst[slot] = vals[orig[slot] - first] for the slots whose original id lies in [first, first+count)
__global__ __launch_bounds__(256) void scatter_by_id(double *__restrict__ dst, const int32_t *__restrict__ orig,
                                                     const double *__restrict__ vals, int64_t n, int64_t first, int64_t count) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = (int64_t)orig[i] - first;
    if (id >= 0 && id < count) dst[i] = vals[id];
}

struct FieldPtrs {
    double *p[SPH_F_COUNT];
    int32_t nf;
};

// out[f][k] = field_f[slot of original id ids[k]]   (ids == nullptr: ids[k] = k)
__global__ __launch_bounds__(256) void gather_by_id(FieldPtrs fp, const int32_t *__restrict__ inv,
                                                    const int64_t *__restrict__ ids, int64_t count,
                                                    double *__restrict__ out) {
    int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const int32_t slot = inv[ids ? ids[k] : k];
    for (int f = 0; f < fp.nf; f++) out[(size_t)f * count + k] = fp.p[f][slot];
}

// the same for a selection whose size only the device knows (sph_select_boxes_async): out[0] = count, out[1] = 0, then
// out[2 + f * count + k] for k < count -- if count <= capacity; else the header alone (the caller asks again, exactly)
__global__ __launch_bounds__(256) void gather_selected(FieldPtrs fp, const int32_t *__restrict__ inv, const int64_t *__restrict__ ids,
                                                       const int64_t *__restrict__ count_ptr, int64_t capacity, double *__restrict__ out) {
    const int64_t count = *count_ptr;
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k == 0) { out[0] = (double)count; out[1] = 0.0; }
    if (k >= count || count > capacity) return;
    const int32_t slot = inv[ids[k]];
    for (int f = 0; f < fp.nf; f++) out[2 + (size_t)f * count + k] = fp.p[f][slot];
}

// field_f[slot of original id first+k] = vals[f][k]
__global__ __launch_bounds__(256) void scatter_many_by_id(FieldPtrs fp, const int32_t *__restrict__ inv, int64_t first,
                                                          int64_t count, const double *__restrict__ vals) {
    int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const int32_t slot = inv[first + k];
    for (int f = 0; f < fp.nf; f++) fp.p[f][slot] = vals[(size_t)f * count + k];
}

}  // namespace

hipError_t launch_gather_fields(sph_ctx *c, int nf, const int *fields, const int64_t *ids, int64_t count, double *out) {
    if (count <= 0 || nf <= 0) return hipSuccess;
    FieldPtrs fp{};
    fp.nf = nf;
    for (int f = 0; f < nf; f++) fp.p[f] = c->f[fields[f]];
    if (hipError_t e = ensure_inv(c); e != hipSuccess) return e;
    gather_by_id<<<dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream>>>(fp, c->inv, ids, count, out);
    return hipGetLastError();
}

hipError_t launch_gather_selected(sph_ctx *c, int nf, const int *fields, int box, int64_t capacity, double *out) {
    FieldPtrs fp{};
    fp.nf = nf;
    for (int f = 0; f < nf; f++) fp.p[f] = c->f[fields[f]];
    const int64_t threads = std::max<int64_t>(capacity, 1);
    if (hipError_t e = ensure_inv(c); e != hipSuccess) return e;
    gather_selected<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c->stream>>>(fp, c->inv, c->sel_ids + (size_t)box * c->sel_stride,
                                                                                        c->sel_count + box, capacity, out);
    return hipGetLastError();
}

hipError_t launch_scatter_fields(sph_ctx *c, int nf, const int *fields, int64_t first, int64_t count, const double *vals) {
    if (count <= 0 || nf <= 0) return hipSuccess;
    FieldPtrs fp{};
    fp.nf = nf;
    for (int f = 0; f < nf; f++) fp.p[f] = c->f[fields[f]];
    if (hipError_t e = ensure_inv(c); e != hipSuccess) return e;
    scatter_many_by_id<<<dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream>>>(fp, c->inv, first, count, vals);
    return hipGetLastError();
}

// A context of one rank without ghosts does not gather by id every step: its reorder leaves inv alone (a scattered 4-byte
// store per particle) and whoever needs inv asks here first.  orig[0, n) is the reorder's own output as long as no ghost
// swap is pending; domain_replace_ghosts asks before it appends.  SPH_NO_LAZY_INV: A/B switch, every reorder stores inv.
hipError_t ensure_inv(sph_ctx *c) {
    if (c->inv_valid) return hipSuccess;
    if (c->n > 0) inv_from_orig<<<dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream>>>(c->orig, c->inv, c->n);
    c->inv_valid = true;
    return hipGetLastError();
}

hipError_t launch_kick_drift_keys(sph_ctx *c) {
    KickDriftArgs a{c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], c->f[SPH_F_VX], c->f[SPH_F_VY], c->f[SPH_F_VZ], c->f[SPH_F_U], c->f[SPH_F_ALPHA],
                    c->f[SPH_F_AX], c->f[SPH_F_AY], c->f[SPH_F_AZ], c->f[SPH_F_DU], c->f[SPH_F_DALPHA]};
    c->early_blocks = (int)std::min<int64_t>((c->n + 255) / 256, EARLY_MAX_BLOCKS);
    kick_drift_keys<<<dim3(c->early_blocks), dim3(256), 0, c->stream>>>(a, c->grid_early, c->n, c->d_dt, c->sink, c->ns, c->keys, c->cell_start,
                                                                        c->bbox_part + BBOX_PART_CLASSIC, c->d_flags);
    return hipGetLastError();
}

hipError_t launch_fill(sph_ctx *c, double *p, double v, int64_t n) {
    if (n <= 0) return hipSuccess;
    fill_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream>>>(p, v, n);
    return hipGetLastError();
}

hipError_t launch_scatter_field(sph_ctx *c, double *field, int64_t first, int64_t count, const double *vals) {
    if (c->n <= 0 || count <= 0) return hipSuccess;
    scatter_by_id<<<dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream>>>(field, c->orig, vals, c->n, first, count);
    return hipGetLastError();
}

hipError_t grid_sort_tmp_bytes(int64_t n, size_t *bytes) {
    size_t b = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (size_t)n, 0u, 32u, (hipStream_t) nullptr);
    *bytes = b;
    return e;
}

hipError_t launch_iota(sph_ctx *c, int32_t *p, int64_t n) {
    if (n <= 0) return hipSuccess;
    iota_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream>>>(p, n);
    return hipGetLastError();
}

hipError_t launch_unpermute(sph_ctx *c, const double *src_sorted, double *dst_original) {
    if (c->n <= 0) return hipSuccess;
    unpermute<<<dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream>>>(src_sorted, c->orig, dst_original, c->n);
    return hipGetLastError();
}

// device-side cell key for the pair kernels lives in pairs.hip (same formula)

// bounding box of the owned particles at their current positions -> d_out6 (device) and/or h_out6 (host, synchronises)
int owned_bbox(sph_ctx *c, double *d_out6, double *h_out6) {
    hipStream_t st = c->stream;
    const int64_t ns = c->n_slots;
    int nb = (int)std::min<int64_t>((ns + BB_BLOCK - 1) / BB_BLOCK, BB_MAX_BLOCKS);
    if (nb < 1) nb = 1;
    double *res = c->bbox_part + (size_t)BB_MAX_BLOCKS * 6 + 8;
    bbox_partial<<<dim3(nb), dim3(BB_BLOCK), 0, st>>>(c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], ns, c->bbox_part, c->d_flags + 2,
                                                      c->orig, (int32_t)c->n_owned, 0, 1);
    bbox_final<<<dim3(1), dim3(384), 0, st>>>(c->bbox_part, nb, res);
    SPH_HIP(hipGetLastError());
    if (d_out6) SPH_HIP(hipMemcpyAsync(d_out6, res, 6 * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (h_out6) {
        SPH_HIP(hipMemcpyAsync(c->pin->owned_box, res, 6 * sizeof(double), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));
        for (int a = 0; a < 6; a++) h_out6[a] = c->pin->owned_box[a];
    }
    return SPH_OK;
}

// the state into the order of c->vals_alt (the sorted slots of the build); n = c->n live entries
static int reorder_sorted(sph_ctx *c, bool ranked = false) {
    const int64_t n = c->n;
    const unsigned gb = (unsigned)((std::max<int64_t>(n, 1) + 255) / 256);
    hipStream_t st = c->stream;
    // ---- reorder state into sorted slots --------------------------------------------------
    ReorderArgs ra{};
    for (int k = 0; k < 9; k++) { ra.src[k] = c->f[k]; ra.dst[k] = c->f_alt[k]; }
    ra.nf = 9; ra.prec = nullptr;
    if (c->variable) { ra.src[9] = c->f[SPH_F_H]; ra.dst[9] = c->f_alt[9]; ra.nf = 10; ra.prec = c->prec; }
    c->inv_valid = switches().no_lazy_inv || c->nranks > 1 || c->n_owned != n;          // SPH_NO_LAZY_INV: A/B switch
    // ranked: c->vals holds the cells' entries in arrival order (cell_scatter); the rank is taken on the way
    if (ranked) reorder_ranked<<<dim3(gb), dim3(256), 0, st>>>(ra, c->keys, c->cell_start, c->vals, c->orig, c->orig_alt, c->inv_valid ? c->inv : nullptr, c->drec, n);
    else reorder<<<dim3(gb), dim3(256), 0, st>>>(ra, c->vals_alt, c->orig, c->orig_alt, c->inv_valid ? c->inv : nullptr, c->drec, n);
    SPH_HIP(hipGetLastError());
    for (int k = 0; k < 9; k++) std::swap(c->f[k], c->f_alt[k]);
    if (c->variable) std::swap(c->f[SPH_F_H], c->f_alt[9]);
    std::swap(c->orig, c->orig_alt);
    c->grid_builds++;
    return SPH_OK;
}

void grid_hash_free(sph_ctx *c) {
    ctx_free(c, c->hkeys); ctx_free(c, c->hkeys_alt); ctx_free(c, c->ukey); ctx_free(c, c->ustart); ctx_free(c, c->uidx);
    ctx_free(c, c->d_m); ctx_free(c, c->htab);
    ctx_free_ptr(c, c->hash_tmp); c->hash_tmp = nullptr;
    c->hash_cap = 0; c->htab_len = 0; c->hash_tmp_bytes = 0; c->hash_bytes = 0;
    c->hv = HashView{};
}

int64_t grid_occupied_cells(const sph_ctx *c) {
    if (!c->hashed) return c->grid.ncells;
    int32_t m = 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(&m, c->d_m, sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return m;
}

// keys, sort, occupied cells and hash table of a hashed grid (c->grid set).  Every buffer is sized from the particle
// capacity, never from the occupied-cell count, which stays on the device: the build adds no read-back.
static int hash_build(sph_ctx *c, bool swap) {
    const GridDesc &g = c->grid;
    const int64_t n = c->n, ns = c->n_slots;
    hipStream_t st = c->stream;
    if (c->hash_cap < c->cap) {
        grid_hash_free(c);
        const int64_t cap = c->cap;
        int64_t tl = 1;
        while (tl < 4 * cap) tl <<= 1;            // two keys per occupied cell at most 2 cap: load factor <= 1/2
        size_t sort_b = 0, scan_b = 0;
        SPH_HIP(rocprim::radix_sort_pairs(nullptr, sort_b, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                          (uint32_t *)nullptr, (size_t)cap, 0u, 64u, st));
        SPH_HIP(rocprim::inclusive_scan(nullptr, scan_b, (int32_t *)nullptr, (int32_t *)nullptr, (size_t)cap, rocprim::plus<int32_t>(), st));
        const int64_t before = c->device_bytes;
        const size_t tmp = std::max(sort_b, scan_b);
        if (ctx_alloc(c, &c->hkeys, (size_t)cap, "hashed grid keys") != SPH_OK ||
            ctx_alloc(c, &c->hkeys_alt, (size_t)cap, "hashed grid keys (alt)") != SPH_OK ||
            ctx_alloc(c, &c->ukey, (size_t)cap + 1, "hashed grid cell keys") != SPH_OK ||
            ctx_alloc(c, &c->ustart, (size_t)cap + 2, "hashed grid cell starts") != SPH_OK ||
            ctx_alloc(c, &c->uidx, (size_t)cap, "hashed grid run index") != SPH_OK ||
            ctx_alloc(c, &c->d_m, 4, "hashed grid cell count") != SPH_OK ||
            ctx_alloc(c, &c->htab, (size_t)tl, "hashed grid table") != SPH_OK ||
            ctx_alloc_bytes(c, &c->hash_tmp, tmp ? tmp : 1, "hashed grid scratch") != SPH_OK) {
            grid_hash_free(c);
            return SPH_ERR_NOMEM;
        }
        c->hash_cap = cap; c->htab_len = tl; c->hash_tmp_bytes = tmp;
        c->hash_bytes = c->device_bytes - before;
    }
    if (c->variable && c->hmax_cap < c->cap + 1) {
        ctx_free(c, c->cell_hmax);
        if (ctx_alloc(c, &c->cell_hmax, (size_t)c->cap + 1, "cell hmax") != SPH_OK) { c->hmax_cap = 0; return SPH_ERR_NOMEM; }
        c->hmax_cap = c->cap + 1;
    }
    int b[3];
    for (int a = 0; a < 3; a++) {
        b[a] = 0;
        while (((int64_t)1 << b[a]) < g.dim[g.s[a]]) b[a]++;
    }
    const int sh1 = b[0], sh2 = b[0] + b[1];
    const unsigned bits = (unsigned)std::max(1, sh2 + b[2] + (swap ? 1 : 0));    // ~0 keys of replaced ghosts: all ones, behind every cell
    const unsigned gbs = (unsigned)((ns + 255) / 256), gb = (unsigned)((std::max<int64_t>(n, 1) + 255) / 256);
    hash_keys<<<dim3(gbs), dim3(256), 0, st>>>(g, sh1, sh2, c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], ns, c->hkeys, c->vals,
                                               c->orig, (int32_t)c->n_owned, c->dead_below);
    SPH_HIP(hipGetLastError());
    size_t tmp = c->hash_tmp_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(c->hash_tmp, tmp, c->hkeys, c->hkeys_alt, c->vals, c->vals_alt, (size_t)ns, 0u, bits, st));
    c->n_slots = n; c->dead_below = 0;     // the replaced ghosts sorted behind the n live entries and are dropped here
    SPH_HIP(hipMemsetAsync(c->d_m, 0, sizeof(int32_t), st));          // no live particle: no cell (hash_compact writes nothing)
    SPH_HIP(hipMemsetAsync(c->ustart, 0, sizeof(int32_t), st));
    if (n > 0) {
        hash_heads<<<dim3(gb), dim3(256), 0, st>>>(c->hkeys_alt, n, c->uidx);
        SPH_HIP(hipGetLastError());
        tmp = c->hash_tmp_bytes;
        SPH_HIP(rocprim::inclusive_scan(c->hash_tmp, tmp, c->uidx, c->uidx, (size_t)n, rocprim::plus<int32_t>(), st));
        hash_compact<<<dim3(gb), dim3(256), 0, st>>>(c->hkeys_alt, c->uidx, n, c->ukey, c->ustart, c->d_m);
    }
    SPH_HIP(hipMemsetAsync(c->htab, 0xff, sizeof(HashEnt) * (size_t)c->htab_len, st));
    hash_insert<<<dim3(gb), dim3(256), 0, st>>>(c->ukey, c->ustart, c->d_m, c->htab, (uint64_t)(c->htab_len - 1));
    SPH_HIP(hipGetLastError());
    c->hv.tab = c->htab; c->hv.ukey = c->ukey; c->hv.ustart = c->ustart; c->hv.m = c->d_m;
    c->hv.mask = (uint64_t)(c->htab_len - 1); c->hv.sh1 = sh1; c->hv.sh2 = sh2;
    return SPH_OK;
}

static bool sort_radix_forced() { return switches().sort_radix; }      // SPH_SORT_RADIX: A/B switch

static bool same_grid(const GridDesc &a, const GridDesc &b) {
    bool same = a.inv_edge == b.inv_edge && a.ncells == b.ncells;
    for (int k = 0; k < 3; k++) same = same && a.org[k] == b.org[k] && a.dim[k] == b.dim[k] && a.s[k] == b.s[k];
    return same;
}

// What grid_rebuild will decide on the host, taken before the opening kick + drift of a step so that this pass can leave the
// keys, the histogram and the box partials behind (launch_kick_drift_keys): the steady state of the plain fixed-h path, where
// the grid comes from the box of the previous build (read-back slot 1 - ring_bbox, which arrived a step ago: the wait below
// is the one grid_rebuild does a few launches later).  Only the build that needs nothing else is taken early -- dense table
// within the capacity in place, no trim, counting sort, no ghosts pending -- and grid_rebuild checks that its own grid is this
// one before it believes the keys.  Zeroes the table and the cursors on the stream; sets c->keys_early.  SPH_NO_DRIFT_KEYS: A/B.
int grid_prepare_early(sph_ctx *c) {
    c->keys_early = false;
    const int64_t n = c->n;
    if (switches().no_drift_keys || n <= 0 || c->n_slots != n || c->dead_below != 0 || c->variable || c->gravity ||
        (c->p.flags & (SPH_FLAG_ACCRETE_CULL | SPH_FLAG_HASHED_GRID)) || !c->ring_bbox_valid || c->no_stale || c->hash_sticky ||
        sort_radix_forced())
        return SPH_OK;
    const int q = 1 - c->ring_bbox;
    SPH_HIP(hipEventSynchronize(c->ev_bbox[q]));
    const double *bb = c->pin->bbox[q].box;
    if (c->pin->bbox[q].nonfinite != 0) return SPH_OK;         // grid_rebuild reports it
    const double guard = 2.0 * c->p.h * (1.0 + 1e-6);
    double box[6];
    for (int a = 0; a < 3; a++) { box[a] = bb[a] - guard; box[3 + a] = bb[3 + a] + guard; }
    GridDesc g{};
    g.inv_edge = 1.0 / (2.0 * c->p.h * (1.0 + 1e-6));
    double ncell_d = 1.0;
    for (int a = 0; a < 3; a++) {
        g.org[a] = box[a];
        const double d = std::floor((box[3 + a] - box[a]) * g.inv_edge) + 1.0;
        if (!(d >= 1.0) || d > 2.0e9) return SPH_OK;
        g.dim[a] = (int32_t)d;
        ncell_d *= d;
    }
    if (ncell_d > 64.0 * (double)n + 4.0e6 || ncell_d >= 2147483647.0) return SPH_OK;       // the trimmed or hashed build
    g.ncells = (int64_t)g.dim[0] * g.dim[1] * g.dim[2];
    int s[3] = {0, 1, 2};
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 3; j++)
            if (g.dim[s[j]] < g.dim[s[i]]) std::swap(s[i], s[j]);
    std::swap(s[1], s[2]);
    g.s[0] = s[0]; g.s[1] = s[1]; g.s[2] = s[2];
    if (g.ncells + 2 > c->cell_cap || g.ncells > 4 * n + 1000000) return SPH_OK;              // table regrown / radix sort
    size_t scan_tmp = 0;
    SPH_HIP(rocprim::exclusive_scan(nullptr, scan_tmp, c->cell_start, c->cell_start, 0, (size_t)(g.ncells + 2), rocprim::plus<int32_t>(), c->stream));
    if (scan_tmp > c->sort_tmp_bytes) return SPH_OK;
    const size_t table = ((size_t)(g.ncells + 2) + 3) & ~(size_t)3, cursors = ((size_t)(g.ncells + 1) + 3) & ~(size_t)3;
    SPH_HIP(hipMemsetAsync(c->cell_start, 0, sizeof(int32_t) * (table + cursors), c->stream));
    c->grid_early = g;
    c->keys_early = true;
    return SPH_OK;
}

int grid_rebuild(sph_ctx *c) {
    const int64_t n = c->n;                 // live particles after the build
    const int64_t ns = c->n_slots;          // occupied slots before it (> n while a ghost swap is pending)
    const bool swap = c->dead_below > 0;
    hipStream_t st = c->stream;
    // keys, histogram and box partials of the current positions are there already (launch_kick_drift_keys)
    bool early = c->keys_early;
    c->keys_early = false;
    if (ns == 0) { c->grid_valid = true; return SPH_OK; }

    // ---- bounding box ---------------------------------------------------------------
    int nb = (int)std::min<int64_t>((ns + BB_BLOCK - 1) / BB_BLOCK, BB_MAX_BLOCKS);
    const int p = c->ring_bbox;
    double *slot = c->pin->bbox[p].box;      // bbox_final writes the whole BoxReport through it
    const bool stale = c->ring_bbox_valid && !c->no_stale && !c->variable && !c->gravity && !(c->p.flags & SPH_FLAG_ACCRETE_CULL);
    early = early && stale && !swap && ns == n;
    auto box_launches = [&]() -> int {
        // d_flags[0] (non-finite position seen) is zero here: cleared at creation and by every bbox_final
        bbox_partial<<<dim3(nb), dim3(BB_BLOCK), 0, st>>>(c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], ns, c->bbox_part, c->d_flags,
                                                          c->orig, (int32_t)c->n_owned, c->dead_below, 0);
        bbox_final<<<dim3(1), dim3(384), 0, st>>>(c->bbox_part, nb, c->bbox_part + (size_t)BB_MAX_BLOCKS * 6, slot, c->d_flags);
        SPH_HIP(hipGetLastError());
        SPH_HIP(hipEventRecord(c->ev_bbox[p], st));        // bbox_final wrote the slot itself (pinned memory)
        return SPH_OK;
    };
    // the exact box of the current positions -> read-back slot p.  Who needs it NOW (octree root boxes: variable h,
    // self-gravity, accretion; the first build of a particle set) waits for it; the plain fixed-h path takes the box of the
    // previous build, which arrived long ago, widened by one cell: particles outside the grid's box are clamped into its
    // boundary cells and still meet all their neighbours there, so the box only has to be roughly right.
    // With the partials of launch_kick_drift_keys in place the box is finished further down, on cell_scatter.
    if (!early) SPH_TRY(box_launches());
    const BoxReport *rep = &c->pin->bbox[p];
    if (stale) {
        SPH_HIP(hipEventSynchronize(c->ev_bbox[1 - p]));
        rep = &c->pin->bbox[1 - p];
    } else {
        SPH_HIP(hipStreamSynchronize(st));
        c->host_syncs++;
    }
    c->ring_bbox = 1 - p; c->ring_bbox_valid = true; c->bbox_exact = !stale;
    const double *bb = rep->box;
    if (rep->nonfinite != 0) {
        c->err = "non-finite particle position at grid build";
        return SPH_ERR_NONFINITE;
    }
    const double guard = stale ? 2.0 * c->p.h * (1.0 + 1e-6) : 0.0;
    for (int a = 0; a < 3; a++) { c->bbox[a] = bb[a] - guard; c->bbox[3 + a] = bb[3 + a] + guard; }
    bb = c->bbox;
    GridDesc g{};
    // fixed h: cells of edge 2h.  variable h: edge 2 <h> with a per-cell maximum of h (varh.hip)
    const double edge = 2.0 * (c->variable ? c->h_mean : c->p.h) * (1.0 + 1e-6);
    g.inv_edge = 1.0 / edge;
    auto cells_of = [&](const double *b) {
        double v = 1.0;
        for (int a = 0; a < 3; a++) v *= std::floor((b[3 + a] - b[a]) * g.inv_edge) + 1.0;
        return v;
    };
    const double sparse_limit = 64.0 * (double)ns + 4.0e6;
    // Dense or hashed.  Dense wherever a dense table can be built (below); hashed when SPH_FLAG_HASHED_GRID asks for it, where
    // the dense table cannot hold the box (fixed h: 2^31 cells after the trim below; variable h: more than 2^27 cells, where
    // the cells used to be widened to many smoothing lengths), and -- once a build had to go hashed -- while the untrimmed box
    // stays sparse: such builds skip the trim rounds and their read-backs.  A hashed grid covers the untrimmed box.
    bool hashed = (c->p.flags & SPH_FLAG_HASHED_GRID) != 0;
    if (!hashed && c->hash_sticky) {
        hashed = cells_of(bb) > sparse_limit;
        if (!hashed) c->hash_sticky = false;
    }
    if (!hashed && c->variable && cells_of(bb) > 134217728.0) hashed = c->hash_sticky = true;
    // Very sparse domains (a particle that escaped to 1e5 AU, a diffuse halo): the cell table must not grow with the
    // VOLUME of the bounding box.  The grid's box need not hold every particle -- a particle outside it is clamped into
    // a boundary cell, where it still meets all its neighbours (cells are >= 2h wide, so everything within 2h of an
    // outside particle is clamped to the same layer or sits in the last one: enough for the fixed-h builds, which scan +-1
    // cell without a distance test; the variable-h build prunes cells by their distance from the particle and therefore
    // treats the boundary cells as open-ended, varh.hip axis_gap2) -- so when the exact box would need more
    // than ~64 cells per particle the grid covers the bulk only: mean +- 6 sigma of the particles inside the current box,
    // trimmed repeatedly (a far outlier inflates sigma, the next round no longer sees it).  Results do not depend on the
    // box beyond summation order; only the boundary cells get crowded if MANY particles lie outside.  A hashed grid trims
    // only the axes that exceed 2^21 cells (the bits of its keys).
    double tb[6] = {bb[0], bb[1], bb[2], bb[3], bb[4], bb[5]};
    auto axis_cells = [&](const double *b, int a) { return std::floor((b[3 + a] - b[a]) * g.inv_edge) + 1.0; };
    const double axis_limit = (double)(1 << HASH_AXIS_BITS);
    auto too_long = [&](const double *b) {
        for (int a = 0; a < 3; a++) if (axis_cells(b, a) > axis_limit) return true;
        return false;
    };
    auto trim = [&](bool for_hash) -> int {
        for (int round = 0; round < 8 && (for_hash ? too_long(tb) : cells_of(tb) > sparse_limit); round++) {
            Box6 bx;
            for (int a = 0; a < 3; a++) { bx.lo[a] = tb[a]; bx.hi[a] = tb[3 + a]; }
            double *mpart = c->bbox_part;                                   // >= 1024 * 7 doubles
            moment_partial<<<dim3(nb), dim3(BB_BLOCK), 0, st>>>(c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], ns, bx, mpart, c->orig,
                                                                (int32_t)c->n_owned, c->dead_below);
            moment_final<<<dim3(1), dim3(448), 0, st>>>(mpart, nb, mpart + (size_t)BB_MAX_BLOCKS * 7);
            SPH_HIP(hipGetLastError());
            SPH_HIP(hipMemcpyAsync(c->pin->trim, mpart + (size_t)BB_MAX_BLOCKS * 7, 7 * sizeof(double), hipMemcpyDeviceToHost, st));
            SPH_HIP(hipStreamSynchronize(st));
            c->host_syncs++;
            const double *mo = c->pin->trim;
            if (!(mo[0] >= 1.0)) break;
            bool shrunk = false;
            for (int a = 0; a < 3; a++) {
                if (for_hash && axis_cells(tb, a) <= axis_limit) continue;
                const double mean = mo[1 + a] / mo[0];
                const double sig = std::sqrt(std::max(mo[4 + a] / mo[0] - mean * mean, 0.0));
                const double half = 6.0 * sig + 2.0 * edge;
                const double lo = std::max(tb[a], mean - half), hi = std::min(tb[3 + a], mean + half);
                if (lo > tb[a] || hi < tb[3 + a]) shrunk = true;
                tb[a] = lo; tb[3 + a] = hi;
            }
            if (!shrunk) break;
        }
        return SPH_OK;
    };
    if (!hashed) {
        { const int st2 = trim(false); if (st2 != SPH_OK) return st2; }
        double ncell_d = 1.0;
        for (int a = 0; a < 3; a++) {
            const double d = std::floor((tb[3 + a] - tb[a]) * g.inv_edge) + 1.0;
            if (!(d >= 1.0)) { c->err = "cell grid dimension out of range"; return SPH_ERR_GRID; }
            ncell_d *= d;
        }
        if (ncell_d >= 2147483647.0) {          // the dense table cannot hold even the trimmed box: hashed, over the whole box
            hashed = c->hash_sticky = true;
            for (int a = 0; a < 6; a++) tb[a] = bb[a];
        }
    }
    if (hashed) { const int st2 = trim(true); if (st2 != SPH_OK) return st2; }
    bb = tb;
    double ncell_d = 1.0;
    for (int a = 0; a < 3; a++) {
        g.org[a] = bb[a];
        double ext = bb[3 + a] - bb[a];
        double d = std::floor(ext * g.inv_edge) + 1.0;
        if (!(d >= 1.0) || d > (hashed ? axis_limit : 2.0e9)) { c->err = "cell grid dimension out of range"; return SPH_ERR_GRID; }
        g.dim[a] = (int32_t)d;
        ncell_d *= d;
    }
    if (!hashed && ncell_d >= 2147483647.0) { c->err = "cell grid exceeds 2^31 cells"; return SPH_ERR_GRID; }
    g.ncells = hashed ? 0 : (int64_t)g.dim[0] * g.dim[1] * g.dim[2];
    c->index_cells = ncell_d;
    // axis permutation: the axis with the fewest cells runs fastest (a column of cells is short: the thin direction of a
    // disc), the LONGEST of the other two is the middle one.  Rows are then as long as possible, a workgroup of consecutive
    // particles rarely wraps from one row into the next, and its three candidate intervals (tiled.hip) stay a few columns
    // wide -- also in the narrow x-slabs of a multi-GPU run, where the short axis in the middle would make every
    // interval span whole rows
    int s[3] = {0, 1, 2};
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 3; j++)
            if (g.dim[s[j]] < g.dim[s[i]]) std::swap(s[i], s[j]);
    std::swap(s[1], s[2]);
    g.s[0] = s[0]; g.s[1] = s[1]; g.s[2] = s[2];
    c->grid = g;
    c->hashed = hashed;
    // the early keys hold for the early grid only; any other decision below (hashed, table regrown, radix sort) drops them too
    if (early && (hashed || !same_grid(g, c->grid_early) || g.ncells + 2 > c->cell_cap)) { early = false; SPH_TRY(box_launches()); }
    if (hashed) {
        const int st2 = hash_build(c, swap);
        if (st2 != SPH_OK) return st2;
        return reorder_sorted(c);
    }

    if (g.ncells + 2 > c->cell_cap) {
        ctx_free(c, c->cell_start); c->cell_fill = nullptr;
        c->cell_cap = (g.ncells + 2) + (g.ncells + 2) / 4;
        // one allocation: the cell table and, right behind the part in use, the cursors of the counting sort (one fill zeroes both)
        if (ctx_alloc(c, &c->cell_start, 2 * (size_t)c->cell_cap + 16, "cell table + cursors") != SPH_OK) { c->cell_cap = 0; return SPH_ERR_NOMEM; }
    }
    if (c->variable && c->hmax_cap < c->cell_cap) {
        ctx_free(c, c->cell_hmax);
        if (ctx_alloc(c, &c->cell_hmax, (size_t)c->cell_cap, "cell hmax") != SPH_OK) { c->hmax_cap = 0; return SPH_ERR_NOMEM; }
        c->hmax_cap = c->cell_cap;
    }

    // ---- keys, sort, cell table ---------------------------------------------------------
    const unsigned gb = (unsigned)((std::max<int64_t>(n, 1) + 255) / 256);
    const unsigned gbs = (unsigned)((ns + 255) / 256);
    size_t scan_tmp = 0;
    bool ranked = false;
    bool counting = !sort_radix_forced() && g.ncells <= 4 * ns + 1000000;
    if (counting) {
        SPH_HIP(rocprim::exclusive_scan(nullptr, scan_tmp, c->cell_start, c->cell_start, 0, (size_t)(g.ncells + 2), rocprim::plus<int32_t>(), st));
        counting = scan_tmp <= c->sort_tmp_bytes;
    }
    if (early && !counting) { early = false; SPH_TRY(box_launches()); }
    if (counting) {
        const size_t table = ((size_t)(g.ncells + 2) + 3) & ~(size_t)3, cursors = ((size_t)(g.ncells + 1) + 3) & ~(size_t)3;
        c->cell_fill = c->cell_start + table;
        if (!early) {
            SPH_HIP(hipMemsetAsync(c->cell_start, 0, sizeof(int32_t) * (table + cursors), st));        // multiples of 16 bytes: one fill kernel
            cell_keys_count<<<dim3(gbs), dim3(256), 0, st>>>(g, c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], ns, c->keys, c->cell_start,
                                                            c->orig, (int32_t)c->n_owned, c->dead_below);
            SPH_HIP(hipGetLastError());
        }
        // in place: cell_start[c] = first sorted slot of cell c; [ncells] = live particles; the replaced ghosts sort behind them
        SPH_HIP(rocprim::exclusive_scan(c->sort_tmp, scan_tmp, c->cell_start, c->cell_start, 0, (size_t)(g.ncells + 2), rocprim::plus<int32_t>(), st));
        if (early) {
            // SPH_NO_BOX_RIDE (A/B switch): the box of the early partials by a launch of its own
            const BoxFinal bf{c->bbox_part + BBOX_PART_CLASSIC, c->early_blocks, c->bbox_part + (size_t)BB_MAX_BLOCKS * 6, slot, c->d_flags};
            if (switches().no_box_ride) {
                bbox_final<<<dim3(1), dim3(384), 0, st>>>(bf.partial, bf.nblocks, bf.out, bf.host_slot, bf.flags);
                cell_scatter<false><<<dim3(gbs), dim3(256), 0, st>>>(c->keys, ns, c->cell_start, c->cell_fill, c->vals, BoxFinal{});
            } else {
                cell_scatter<true><<<dim3(gbs + 1), dim3(256), 0, st>>>(c->keys, ns, c->cell_start, c->cell_fill, c->vals, bf);
            }
            SPH_HIP(hipGetLastError());
            SPH_HIP(hipEventRecord(c->ev_bbox[p], st));
        } else {
            cell_scatter<false><<<dim3(gbs), dim3(256), 0, st>>>(c->keys, ns, c->cell_start, c->cell_fill, c->vals, BoxFinal{});
        }
        // SPH_NO_RANK_REORDER (A/B switch): the rank by a launch of its own, as every other configuration has it
        ranked = early && !switches().no_rank_reorder;
        if (!ranked) cell_rank<<<dim3(gb), dim3(256), 0, st>>>(c->keys, n, c->cell_start, c->vals, c->vals_alt);
        SPH_HIP(hipGetLastError());
        c->n_slots = n; c->dead_below = 0;
    } else {
        cell_keys<<<dim3(gbs), dim3(256), 0, st>>>(g, c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], ns, c->keys,
                                                  c->vals, c->orig, (int32_t)c->n_owned, c->dead_below);
        SPH_HIP(hipGetLastError());
        unsigned bits = 1;
        while (bits < 32 && ((int64_t)1 << bits) < g.ncells + (swap ? 1 : 0)) bits++;
        size_t tmp = c->sort_tmp_bytes;
        SPH_HIP(rocprim::radix_sort_pairs(c->sort_tmp, tmp, c->keys, c->keys_alt, c->vals, c->vals_alt, (size_t)ns, 0u, bits, st));
        c->n_slots = n; c->dead_below = 0;     // the replaced ghosts sorted behind the n live entries and are dropped here
        cell_table<<<dim3((unsigned)((g.ncells + 1 + 255) / 256)), dim3(256), 0, st>>>(c->keys_alt, n, g.ncells, c->cell_start);
        SPH_HIP(hipGetLastError());
    }

    return reorder_sorted(c, ranked);
}

}  // namespace sph
