// history.hip -- the per-step time series of a context (include/summersph.h, sph_history): one row of doubles per recorded
// step, written into a device-resident log by kernels on the context's stream.  The host keeps the row index, the step
// number and the dropped count; a recorded step waits for nothing and reads nothing back.
//
// Only reads the context: the state, the grid, the list, the statistics, dt and every validity flag stay as they are, and
// with no history begun the step enqueues exactly what it enqueued before.
//
// The gas sums of a row are exact (exact_sum.hpp): each term is sph_energy's fp64 value (energy_terms.hpp), rounded
// half-even to a multiple of 2^(e - 62) with 2^e above the largest |term| of its sum, added in 128-bit integers and
// converted once.  They do not depend on the sorted order, so the passes run over the sorted SoA fields with coalesced
// reads instead of through inv.
//
// Four launches per recorded row, all on ctx->stream:
//   history_maxima   every slot of the owned gas: per-block max |term| of the 13 sums and of v.v, the non-finite marks, and
//                    the densest particle (ties: the lowest original id)
//   history_head     one block, a wavefront per maximum: the partials -> Head: the 13 exponents, the marks, max v.v, the
//                    densest particle
//   history_sums     every slot again (from the cache at the sizes a step runs at): 13 {lo, hi} accumulators per lane in
//                    registers, no atomics; the lanes by a butterfly of 128-bit additions, the waves through LDS, one
//                    26-word partial per block
//   history_row      one block, a wavefront per sum: adds the partials and converts the limbs; further wavefronts: the sink
//                    part (energy_terms.hpp), the sink states, d_dt and the rest -> the row
#include <cmath>
#include <cstring>

#include "energy_terms.hpp"
#include "exact_sum.hpp"
#include "reduce_common.hpp"

// every term in sph_energy's documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int HB = 256;                    // block of the two passes over the particles
constexpr int H_BLOCKS = 1024;             // their blocks at most (grid-stride beyond)
constexpr int NX = 13;                     // exact sums: sph_energy's 1 .. 12 and 14
constexpr int NMX = NX + 1;                // maxima of the first pass: those 13 |term| and v.v
constexpr int BAD_V2 = NX;                 // bit of the marks: a v.v is NaN
constexpr int ROW_E = 6;                   // row index of sph_energy's sums[0]
static_assert(ROW_E + SPH_ENERGY_NSUM + 6 == SPH_HISTORY_NHEAD, "the head of a row");

// exact sum j -> its index in sph_energy's sums
__host__ __device__ constexpr int sum_index(int j) { return j < 12 ? j + 1 : 14; }

struct Fields {
    const double *x, *y, *z, *vx, *vy, *vz, *u, *m;
    const double *rho;                     // null: the density is not current
    const int32_t *orig;
};

struct Head {
    int32_t exps[NX];                      // e_j (0 for a sum with a non-finite term)
    uint32_t bad;                          // bit j: sum j has a non-finite term; bit BAD_V2
    double v2max, rho;
    int32_t id, slot;                      // the densest particle (slot < 0: none)
};

// is the particle {r, id} denser than {rb, idb} (ties: the lower id)?  NaN is never denser
__device__ __forceinline__ bool denser(double r, int32_t id, double rb, int32_t idb) { return r > rb || (r == rb && id < idb); }

// the 13 exact terms and v.v of slot i
__device__ __forceinline__ void slot_terms(const Fields &f, int64_t i, const double *__restrict__ sink, int ns, double G,
                                           double (&t)[NX], double &v2) {
    const double x = f.x[i], y = f.y[i], z = f.z[i], vx = f.vx[i], vy = f.vy[i], vz = f.vz[i], m = f.m[i];
    double q[ENERGY_NG];
    gas_terms(x, y, z, vx, vy, vz, f.u[i], m, 0.0, phi_sink(x, y, z, sink, ns, G), q);
#pragma unroll
    for (int j = 0; j < NX; j++) t[j] = q[sum_index(j)];
    v2 = (vx * vx + vy * vy) + vz * vz;
}

__global__ __launch_bounds__(HB) void history_maxima(Fields f, int64_t n_slots, int64_t n_owned,
                                                     const double *__restrict__ sink, int ns, double G,
                                                     double *__restrict__ part, uint32_t *__restrict__ bad_part,
                                                     double *__restrict__ rho_part, int32_t *__restrict__ who_part) {
    __shared__ uint32_t s_bad[HB / WAVE];
    __shared__ double s_rho[HB / WAVE];
    __shared__ int32_t s_id[HB / WAVE], s_slot[HB / WAVE];
    double v[NMX];
#pragma unroll
    for (int k = 0; k < NMX; k++) v[k] = -INFINITY;
    uint32_t bad = 0;
    double rb = -INFINITY;
    int32_t idb = 0x7fffffff, slotb = -1;
    for (int64_t i = (int64_t)blockIdx.x * HB + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * HB) {
        const int32_t id = f.orig[i];
        if (id < 0 || id >= n_owned) continue;            // ghosts and replaced ghosts
        double t[NX], v2;
        slot_terms(f, i, sink, ns, G, t, v2);
#pragma unroll
        for (int j = 0; j < NX; j++) {
            v[j] = fmax(v[j], fabs(t[j]));
            if (!finite(t[j])) bad |= 1u << j;
        }
        v[NX] = fmax(v[NX], v2);
        if (v2 != v2) bad |= 1u << BAD_V2;
        if (f.rho) {
            const double r = f.rho[i];
            if (denser(r, id, rb, idb)) { rb = r; idb = id; slotb = (int32_t)i; }
        }
    }
    bad = wave_or(bad);
    for (int o = 32; o > 0; o >>= 1) {
        const double r = __shfl_xor(rb, o, 64);
        const int32_t id = __shfl_xor(idb, o, 64), sl = __shfl_xor(slotb, o, 64);
        if (denser(r, id, rb, idb)) { rb = r; idb = id; slotb = sl; }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { s_bad[wv] = bad; s_rho[wv] = rb; s_id[wv] = idb; s_slot[wv] = slotb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < HB / WAVE; w++) {
            bad |= s_bad[w];
            if (denser(s_rho[w], s_id[w], rb, idb)) { rb = s_rho[w]; idb = s_id[w]; slotb = s_slot[w]; }
        }
        bad_part[blockIdx.x] = bad;
        rho_part[blockIdx.x] = rb;
        who_part[2 * blockIdx.x] = idb;
        who_part[2 * blockIdx.x + 1] = slotb;
    }
    stats_block_partial<0, NMX, HB, NMX>(v, part);
}

// One block of FW wavefronts, no wave waits for another: wave k < NMX joins maximum k over the blocks (and the marks, which
// decide its exponent), wave NMX the densest particle.  A lane's partials are read in one unrolled batch of loads.
constexpr int FW = 16;                     // wavefronts of the two final kernels
constexpr int PER_LANE = H_BLOCKS / WAVE;  // partials per lane at most
static_assert(NMX + 1 <= FW && NX + 3 <= FW, "a wavefront per piece of the final kernels");

__global__ __launch_bounds__(FW * WAVE) void history_head(const double *__restrict__ part, const uint32_t *__restrict__ bad_part,
                                                          const double *__restrict__ rho_part,
                                                          const int32_t *__restrict__ who_part, int nb, Head *__restrict__ head) {
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    if (k < NMX) {
        double v = -INFINITY;
        uint32_t bad = 0;
#pragma unroll
        for (int it = 0; it < PER_LANE; it++) {
            const int b = lane + it * WAVE;
            if (b < nb) { v = fmax(v, part[b * NMX + k]); bad |= bad_part[b]; }
        }
        v = wave_max(v);
        bad = wave_or(bad);
        if (lane != 0) return;
        if (k < NX) {
            head->exps[k] = (bad >> k & 1u) ? 0 : exp_above(fmax(v, 0.0));    // no gas: the maxima are 0
        } else {
            head->v2max = fmax(v, 0.0);
            head->bad = bad;
        }
    } else if (k == NMX) {
        double rb = -INFINITY;
        int32_t idb = 0x7fffffff, slotb = -1;
#pragma unroll
        for (int it = 0; it < PER_LANE; it++) {
            const int b = lane + it * WAVE;
            if (b < nb) {
                const double r = rho_part[b];
                const int32_t id = who_part[2 * b];
                if (denser(r, id, rb, idb)) { rb = r; idb = id; slotb = who_part[2 * b + 1]; }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double r = __shfl_xor(rb, o, 64);
            const int32_t id = __shfl_xor(idb, o, 64), sl = __shfl_xor(slotb, o, 64);
            if (denser(r, id, rb, idb)) { rb = r; idb = id; slotb = sl; }
        }
        if (lane != 0) return;
        head->rho = rb;
        head->id = idb;
        head->slot = slotb;
    }
}

__global__ __launch_bounds__(HB) void history_sums(Fields f, int64_t n_slots, int64_t n_owned, const double *__restrict__ sink,
                                                   int ns, double G, const Head *__restrict__ head,
                                                   unsigned long long *__restrict__ part) {
    __shared__ unsigned long long sm[HB / WAVE][2 * NX];
    int sh[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) sh[j] = 62 - head->exps[j];
    unsigned long long lo[NX], hi[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) lo[j] = hi[j] = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * HB + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * HB) {
        const int32_t id = f.orig[i];
        if (id < 0 || id >= n_owned) continue;
        double t[NX], v2;
        slot_terms(f, i, sink, ns, G, t, v2);
#pragma unroll
        for (int j = 0; j < NX; j++) add_fixed(lo[j], hi[j], to_fixed(t[j], sh[j]));
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NX; j++) {
        wave_add_limbs(lo[j], hi[j]);
        if (lane == 0) { sm[wv][2 * j] = lo[j]; sm[wv][2 * j + 1] = hi[j]; }
    }
    __syncthreads();
    if (threadIdx.x < NX) {
        const int j = threadIdx.x;
        unsigned long long l = sm[0][2 * j], h = sm[0][2 * j + 1];
        for (int w = 1; w < HB / WAVE; w++) add_limbs(l, h, sm[w][2 * j], sm[w][2 * j + 1]);
        part[((size_t)blockIdx.x * NX + j) * 2] = l;
        part[((size_t)blockIdx.x * NX + j) * 2 + 1] = h;
    }
}

// One block of FW wavefronts, each writing its own entries of the row: wave j < NX adds the partials of sum j (lane-strided in
// one unrolled batch of loads, then the butterfly) and converts the limbs; wave NX the sink part; wave NX + 1 the sink
// states; wave NX + 2 the rest of the head
__global__ __launch_bounds__(FW * WAVE) void history_row(const unsigned long long *__restrict__ part, int nb,
                                                         const Head *__restrict__ head, Fields f, const double *__restrict__ sink,
                                                         int ns, int rank0, double G, const double *__restrict__ d_dt,
                                                         double step, double n_gas, int max_sinks, double *__restrict__ row) {
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
    if (j < NX) {
        unsigned long long lo = 0ull, hi = 0ull;
#pragma unroll
        for (int it = 0; it < PER_LANE; it++) {
            const int b = lane + it * WAVE;
            if (b < nb) add_limbs(lo, hi, part[((size_t)b * NX + j) * 2], part[((size_t)b * NX + j) * 2 + 1]);
        }
        wave_add_limbs(lo, hi);
        if (lane == 0) row[ROW_E + sum_index(j)] = (head->bad >> j & 1u) ? (double)NAN : limbs_to_double(lo, hi, head->exps[j]);
    } else if (j == NX) {
        double sk[ENERGY_NK];
        sink_sums(lane, sink, ns, rank0, G, sk);
        if (lane != 0) return;
#pragma unroll
        for (int s = 0; s < ENERGY_NK; s++) row[ROW_E + ENERGY_NG + s] = sk[s];
    } else if (j == NX + 1) {
        for (int s = lane; s < max_sinks; s += WAVE)
#pragma unroll
            for (int k = 0; k < 7; k++) row[SPH_HISTORY_NHEAD + 7 * s + k] = s < ns ? sink[k * MAX_SINKS + s] : (double)NAN;
    } else if (j == NX + 2 && lane == 0) {
        row[0] = step;
        row[1] = d_dt[1];
        row[2] = d_dt[0];
        row[3] = d_dt[2];
        row[4] = n_gas;
        row[5] = (double)ns;
        row[ROW_E] = n_gas;
        row[ROW_E + 13] = 0.0;                           // W_self: no tree walk here
        const int32_t slot = f.rho ? head->slot : -1;
        row[34] = slot >= 0 ? head->rho : (double)NAN;
        row[35] = slot >= 0 ? (double)head->id : (double)NAN;
        row[36] = slot >= 0 ? f.x[slot] : (double)NAN;
        row[37] = slot >= 0 ? f.y[slot] : (double)NAN;
        row[38] = slot >= 0 ? f.z[slot] : (double)NAN;
        row[39] = (head->bad >> BAD_V2 & 1u) ? (double)NAN : sqrt(head->v2max);
    }
}

}  // namespace

struct History {
    sph_history_desc d{};
    int32_t width = 0;
    int64_t rows = 0, dropped = 0, steps = 0;
    double *log = nullptr;
    double *part = nullptr, *rho_part = nullptr;         // history_maxima's partials
    uint32_t *bad_part = nullptr;
    int32_t *who_part = nullptr;
    Head *head = nullptr;
    unsigned long long *sum_part = nullptr;              // history_sums' partials
};

void history_free(sph_ctx *c) {
    History *h = c->hist;
    if (!h) return;
    ctx_free(c, h->log); ctx_free(c, h->part); ctx_free(c, h->rho_part); ctx_free(c, h->bad_part); ctx_free(c, h->who_part);
    ctx_free(c, h->head); ctx_free(c, h->sum_part);
    delete h;
    c->hist = nullptr;
}

int history_begin(sph_ctx *c, const sph_history_desc *d) {
    const char *who = "sph_history_begin";
    if (!d) return arg_error(c, who, "null descriptor");
    if (d->capacity < 1) return arg_error(c, who, "capacity must be >= 1");
    if (d->every < 1) return arg_error(c, who, "every must be >= 1");
    if (d->max_sinks < 0 || d->max_sinks > MAX_SINKS) return arg_error(c, who, "max_sinks must be 0 .. 64");
    if (d->flags != 0) return arg_error(c, who, "flags must be 0");
    history_free(c);
    History *h = new (std::nothrow) History();
    if (!h) { c->err = "sph_history_begin: out of host memory"; return SPH_ERR_NOMEM; }
    c->hist = h;
    h->d = *d;
    h->width = SPH_HISTORY_NHEAD + 7 * d->max_sinks;
    int st = ctx_alloc(c, &h->log, (size_t)d->capacity * (size_t)h->width, "history log");
    if (st == SPH_OK) st = ctx_alloc(c, &h->part, (size_t)H_BLOCKS * NMX, "history maxima");
    if (st == SPH_OK) st = ctx_alloc(c, &h->rho_part, (size_t)H_BLOCKS, "history densest");
    if (st == SPH_OK) st = ctx_alloc(c, &h->bad_part, (size_t)H_BLOCKS, "history marks");
    if (st == SPH_OK) st = ctx_alloc(c, &h->who_part, (size_t)H_BLOCKS * 2, "history densest ids");
    if (st == SPH_OK) st = ctx_alloc(c, &h->head, 1, "history head");
    if (st == SPH_OK) st = ctx_alloc(c, &h->sum_part, (size_t)H_BLOCKS * NX * 2, "history partial sums");
    if (st != SPH_OK) history_free(c);
    return st;
}

int history_end(sph_ctx *c) {
    if (!c->hist) { c->err = "sph_history_end: no history begun"; return SPH_ERR_STATE; }
    history_free(c);
    return SPH_OK;
}

// appends the row of the state as it is now; a full log drops it and counts
static int history_append(sph_ctx *c) {
    History *h = c->hist;
    if (h->rows >= h->d.capacity) { h->dropped++; return SPH_OK; }
    hipStream_t st = c->stream;
    const int64_t n_slots = c->cap > 0 ? c->n_slots : 0;
    const bool rho_ok = n_slots > 0 && field_ready(*c, c->variable, SPH_F_RHO);
    const Fields f{c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], c->f[SPH_F_VX], c->f[SPH_F_VY], c->f[SPH_F_VZ], c->f[SPH_F_U],
                   c->f[SPH_F_M], rho_ok ? c->f[SPH_F_RHO] : nullptr, c->orig};
    const int nb = (int)std::min<int64_t>(blocks(n_slots, HB), H_BLOCKS);
    double *row = h->log + (size_t)h->rows * (size_t)h->width;
    history_maxima<<<dim3((unsigned)nb), dim3(HB), 0, st>>>(f, n_slots, c->n_owned, c->sink, c->ns, c->p.G, h->part, h->bad_part,
                                                          h->rho_part, h->who_part);
    history_head<<<dim3(1), dim3(FW * WAVE), 0, st>>>(h->part, h->bad_part, h->rho_part, h->who_part, nb, h->head);
    history_sums<<<dim3((unsigned)nb), dim3(HB), 0, st>>>(f, n_slots, c->n_owned, c->sink, c->ns, c->p.G, h->head, h->sum_part);
    history_row<<<dim3(1), dim3(FW * WAVE), 0, st>>>(h->sum_part, nb, h->head, f, c->sink, c->ns, c->rank == 0 ? 1 : 0, c->p.G, c->d_dt,
                                                (double)h->steps, (double)(n_slots > 0 ? c->n_owned : 0), h->d.max_sinks, row);
    SPH_HIP(hipGetLastError());
    h->rows++;
    return SPH_OK;
}

int history_record(sph_ctx *c) {
    if (!c->hist) { c->err = "sph_history_record: no history begun"; return SPH_ERR_STATE; }
    return history_append(c);
}

int history_step(sph_ctx *c) {
    History *h = c->hist;
    if (!h) return SPH_OK;
    h->steps++;
    if (h->steps % h->d.every != 0) return SPH_OK;
    return history_append(c);
}

int history_info(sph_ctx *c, int64_t *rows, int64_t *dropped, int64_t *steps, int32_t *width) {
    const History *h = c->hist;
    if (!h) { c->err = "sph_history_info: no history begun"; return SPH_ERR_STATE; }
    if (rows) *rows = h->rows;
    if (dropped) *dropped = h->dropped;
    if (steps) *steps = h->steps;
    if (width) *width = h->width;
    return SPH_OK;
}

int history_read(sph_ctx *c, int64_t first, int64_t count, double *out, bool host) {
    const char *who = host ? "sph_history_read" : "sph_history_read_dev";
    const History *h = c->hist;
    if (!h) { c->err = std::string(who) + ": no history begun"; return SPH_ERR_STATE; }
    if (first < 0 || count < 0 || first > h->rows || count > h->rows - first) return arg_error(c, who, "first / count outside [0, rows]");
    if (!out && count > 0) return arg_error(c, who, "null output");
    if (count > 0)
        SPH_HIP(hipMemcpyAsync(out, h->log + (size_t)first * (size_t)h->width, (size_t)count * (size_t)h->width * sizeof(double),
                               host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    return SPH_OK;
}

}  // namespace sph
