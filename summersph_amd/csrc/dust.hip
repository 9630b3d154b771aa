// dust.hip -- drag-coupled tracer grains advanced with the run (include/summersph.h, sph_dust): M massless test grains on the
// device, each with a position, a velocity and one drag parameter.  From sph_dust_begin to sph_dust_end every `every`-th step
// advances the live grains from their own clock t_d to the gas clock d_dt[1] by one kick-drift-kick step: the kicks are the
// exact solution of dv/dt = a - r (v - vg) with the sinks' acceleration a, the gas velocity vg and the drag rate r frozen,
// the gas being sampled once per advance, at the new position, in the state the step just left.
//
// Only reads the context: the state, the grid, the list, the statistics, dt and every validity flag stay as they are, and
// with no dust begun the step enqueues exactly what it enqueued before.  An advance waits for nothing and reads nothing back.
//
// The gas a grain sees is sph_sample's, bit for bit: the search structure is sample_build's (sample.hip) over the owned gas,
// mass-weighted, with the rows vx vy vz u and no clip box, and one lane per grain calls point_sums (sample_common.hpp).
//
// An advance (all on ctx->stream):
//   sample_build      select -> levels -> keys -> sort -> records -> tails, with K = 4 rows
//   dust_kick_drift   one lane per grain: the half kick with the stored sample, the drift, the fates, the grain's sort key
//   rocprim radix sort   the grains by their cell in the most populated level (sample_point_keys' rule): only the work
//                     distribution depends on it
//   dust_walk<PER_H>  one lane per grain of the walk order: point_sums at the new position, the drag rate, the sinks'
//                     acceleration in sink order, the second half kick, the stored sample and the row's columns
//   dust_head         one lane: the row's head and the grains' clock
// A grain's result depends on the gas, the sinks, its own state and the interval alone: no float atomics, no sum split
// over lanes.  What the advance keeps between calls is the dust's own memory; the analysis scratch is free again afterwards.
#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <new>
#include <vector>

// the scheme is written in one documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

#include "sample_common.hpp"

namespace sph {

namespace {

constexpr int KB = 256;                    // block of the kick-drift kernel
constexpr int TB = WAVE;                   // block of the walk: one wavefront (trace_walk's choice: a grain in a dense cell
                                           // holds back 63 others at most)
constexpr int NCOL = SPH_DUST_NCOL, NHEAD = SPH_DUST_NHEAD;
constexpr int NST = 7;                     // the state's arrays: x y z vx vy vz par
constexpr int NS = 7;                      // the stored sample's arrays: ax ay az vgx vgy vgz r
constexpr int FATE_ACCRETED = 1, FATE_CULLED = 2, FATE_NONFINITE = 3;

// the exact solution of dv/dt = a - r (v - vg) over tau with a, vg and r frozen
__device__ __forceinline__ void half_kick(double (&v)[3], const double (&a)[3], const double (&vg)[3], double r, double tau) {
    const double k = r * tau;
    if (k > 0.0) {
        const double e = -expm1(-k);
        const double f = tau * (e / k);
#pragma unroll
        for (int i = 0; i < 3; i++) v[i] = (v[i] + (vg[i] - v[i]) * e) + a[i] * f;
    } else if (r == 0.0) {
#pragma unroll
        for (int i = 0; i < 3; i++) v[i] = v[i] + a[i] * tau;
    }
}

__device__ __forceinline__ bool moves(double delta) { return delta > 0.0 && delta <= SAMPLE_DBL_BIG; }

// one integer atomic per wavefront for the grains that left in this launch
__device__ __forceinline__ void count_gone(bool gone, int32_t *__restrict__ live) {
    const unsigned long long hit = __ballot(gone);
    if ((threadIdx.x & (WAVE - 1)) == 0 && hit) atomicSub(live, (int32_t)__popcll(hit));
}

// st: NST arrays of m; smp: NS arrays of m; fates: {fate, advance, sink} per grain; clk: {t_d, the interval of this advance}
__global__ __launch_bounds__(KB) void dust_kick_drift(int64_t m, double *__restrict__ st, const double *__restrict__ smp,
                                                      int32_t *__restrict__ fates, const double *__restrict__ d_dt,
                                                      double *__restrict__ clk, const double *__restrict__ sink,
                                                      const double *__restrict__ sink_radius, int ns, double bound, int remove,
                                                      int32_t advance, const Info *__restrict__ info,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                      int32_t *__restrict__ live) {
    const int64_t p = (int64_t)blockIdx.x * KB + threadIdx.x;
    const bool in = p < m;
    const double delta = d_dt[1] - clk[0];
    if (p == 0) clk[1] = delta;                              // nobody reads clk[1] in this launch
    bool gone = false;
    if (in) {
        uint64_t key = POINT_KEY_NONE;
        if (fates[3 * p] == 0) {
            double x[3], v[3];
#pragma unroll
            for (int i = 0; i < 3; i++) { x[i] = st[i * m + p]; v[i] = st[(3 + i) * m + p]; }
            int fate = 0, by = -1;
            if (moves(delta)) {
                double a[3], vg[3];
#pragma unroll
                for (int i = 0; i < 3; i++) { a[i] = smp[i * m + p]; vg[i] = smp[(3 + i) * m + p]; }
                half_kick(v, a, vg, smp[6 * m + p], 0.5 * delta);
#pragma unroll
                for (int i = 0; i < 3; i++) x[i] = x[i] + v[i] * delta;
                if (remove) {
                    for (int k = 0; k < ns && fate == 0; k++) {
                        const double dx = x[0] - sink[k], dy = x[1] - sink[MAX_SINKS + k], dz = x[2] - sink[2 * MAX_SINKS + k];
                        if (sqrt((dx * dx + dy * dy) + dz * dz) < sink_radius[k]) { fate = FATE_ACCRETED; by = k; }
                    }
                    if (fate == 0 && (fabs(x[0]) > bound || fabs(x[1]) > bound || fabs(x[2]) > bound)) fate = FATE_CULLED;
                }
#pragma unroll
                for (int i = 0; i < 3; i++) { st[i * m + p] = x[i]; st[(3 + i) * m + p] = v[i]; }
            }
            if (!finite3(x[0], x[1], x[2]) || !finite3(v[0], v[1], v[2])) { fate = FATE_NONFINITE; by = -1; }
            if (fate != 0) {
                fates[3 * p] = fate; fates[3 * p + 1] = advance; fates[3 * p + 2] = by;
                gone = true;
            } else {
                key = point_sort_key(info, x[0], x[1], x[2]);
            }
        }
        keys[p] = key;
        vals[p] = (uint32_t)p;
    }
    count_gone(gone, live);
}

struct DustConst {
    double G, gg;                          // gg = gamma * gamma_m1: c^2 = gg u (density_epilogue's EOS)
    double cE, rho_grain;
    int32_t law, ns, advance;
};

// one lane per grain (the t-th in walk order: grain pidx[t]); body: the row's NCOL columns of m, or null
template <bool PER_H>
__global__ __launch_bounds__(TB) void dust_walk(const uint32_t *__restrict__ pidx, int64_t m, SampleView sv, double h_one,
                                                double *__restrict__ st, double *__restrict__ smp, int32_t *__restrict__ fates,
                                                const double *__restrict__ clk, const double *__restrict__ sink, DustConst dc,
                                                int32_t *__restrict__ live, double *__restrict__ body) {
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    const bool in = t < m;
    const int64_t idx = in ? (int64_t)pidx[t] : 0;
    const bool alive = in && fates[3 * idx] == 0;
    const Info *__restrict__ info = sv.info;
    double p[3] = {0.0, 0.0, 0.0};
    if (alive) { p[0] = st[idx]; p[1] = st[m + idx]; p[2] = st[2 * m + idx]; }
    double den = 0.0, num[4] = {0.0, 0.0, 0.0, 0.0};
    const double ih_one = 1.0 / h_one;                       // one h: the records' 1 / h_j, bitwise
    point_sums<4, PER_H>(info, sv.rec, sv.wsa, sv.tab, sv.mask, alive ? info->nlev : 0, p, ih_one, den, num);
    bool gone = false;
    if (alive) {
        double vg[3] = {0.0, 0.0, 0.0}, ug = 0.0, r = 0.0;
        const double par = st[6 * m + idx];
        if (den != 0.0) {
#pragma unroll
            for (int i = 0; i < 3; i++) vg[i] = num[i] / den;
            ug = num[3] / den;
            if (dc.law == SPH_DUST_EPSTEIN) {
                const double cs = sqrt(dc.gg * ug);
                r = ((den * cs) * dc.cE) / (dc.rho_grain * par);
            } else {
                r = 1.0 / par;
            }
        }
        // the sinks in sink order, sph_gravity_at's arithmetic (unsoftened)
        double a[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < dc.ns; k++) {
            const double sm = sink[6 * MAX_SINKS + k];
            if (sm == 0.0) continue;
            const double dx = p[0] - sink[k], dy = p[1] - sink[MAX_SINKS + k], dz = p[2] - sink[2 * MAX_SINKS + k];
            const double rr = sqrt((dx * dx + dy * dy) + dz * dz);
            const double gm = dc.G * sm;
            const double f = gm / ((rr * rr) * rr);
            a[0] = a[0] - f * dx; a[1] = a[1] - f * dy; a[2] = a[2] - f * dz;
        }
        double v[3] = {st[3 * m + idx], st[4 * m + idx], st[5 * m + idx]};
        const double delta = clk[1];
        if (moves(delta)) half_kick(v, a, vg, r, 0.5 * delta);
        gone = info->bad != 0 || !finite3(v[0], v[1], v[2]) || !finite3(a[0], a[1], a[2]);
        if (gone) {
            fates[3 * idx] = FATE_NONFINITE; fates[3 * idx + 1] = dc.advance; fates[3 * idx + 2] = -1;
        } else {
#pragma unroll
            for (int i = 0; i < 3; i++) {
                st[(3 + i) * m + idx] = v[i];
                smp[i * m + idx] = a[i];
                smp[(3 + i) * m + idx] = vg[i];
            }
            smp[6 * m + idx] = r;
            if (body) {
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    body[i * m + idx] = p[i];
                    body[(3 + i) * m + idx] = v[i];
                    body[(8 + i) * m + idx] = vg[i];
                }
                body[6 * m + idx] = den;
                body[7 * m + idx] = ug;
                body[11 * m + idx] = r;
            }
        }
    }
    count_gone(gone, live);
}

// after the walk: the head of the row (null: none) and the grains' clock
__global__ void dust_head(const double *__restrict__ d_dt, double *__restrict__ clk, const int32_t *__restrict__ live,
                          double advance, double *__restrict__ head) {
    if (head) {
        head[0] = advance;
        head[1] = d_dt[1];
        head[2] = clk[1];
        head[3] = (double)*live;
    }
    clk[0] = d_dt[1];
}

}  // namespace

struct Dust {
    sph_dust_desc d{};
    int64_t M = 0;
    int64_t rows = 0, dropped = 0, advances = 0, stepped = 0, steps = 0;
    bool closed = false;
    double cE = 0.0;
    double *head = nullptr, *body = nullptr;             // capacity x NHEAD, capacity x NCOL x M
    double *st = nullptr, *smp = nullptr, *clk = nullptr; // NST x M, NS x M, {t_d, interval}
    int32_t *fates = nullptr, *live = nullptr;
};

void dust_free(sph_ctx *c) {
    Dust *t = c->dust;
    if (!t) return;
    ctx_free(c, t->head); ctx_free(c, t->body); ctx_free(c, t->st); ctx_free(c, t->smp); ctx_free(c, t->clk);
    ctx_free(c, t->fates); ctx_free(c, t->live);
    delete t;
    c->dust = nullptr;
}

void dust_close(sph_ctx *c) { if (c->dust) c->dust->closed = true; }

// one advance to the clock now; record: append its row (a full log drops it and counts)
static int dust_run(sph_ctx *c, const char *who, bool record) {
    Dust *t = c->dust;
    hipStream_t st = c->stream;
    const int64_t m = t->M;
    const bool per_h = c->variable;
    const double h_one = c->variable ? 0.0 : c->p.h;
    if (!per_h && !(h_one > 0.0)) {
        c->err = std::string(who) + ": params.h <= 0 on a fixed-h context";
        return SPH_ERR_STATE;
    }
    const unsigned key_bits = (unsigned)(3 * LEVEL_AXIS_BITS + 1);
    size_t psort_bytes = 0;
    SPH_HIP(rocprim::radix_sort_pairs(nullptr, psort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)m, 0u, key_bits, st));
    uint64_t *pkeys, *pkeys_alt;
    uint32_t *pvals, *pvals_alt;
    auto layout = [&](Carve cv) {
        pkeys = cv.take<uint64_t>(m);
        pkeys_alt = cv.take<uint64_t>(m);
        pvals = cv.take<uint32_t>(m);
        pvals_alt = cv.take<uint32_t>(m);
        return cv.bytes;
    };
    static const double no_lo[3] = {-INFINITY, -INFINITY, -INFINITY}, no_hi[3] = {INFINITY, INFINITY, INFINITY};
    static const int32_t fields[4] = {SPH_F_VX, SPH_F_VY, SPH_F_VZ, SPH_F_U};
    const SampleSources src{no_lo, no_hi, h_one, per_h, false, false, 4, fields, nullptr, psort_bytes};
    SampleView sv{};
    char *extra = nullptr, *sort_tmp = nullptr;
    SPH_TRY(sample_build(c, src, layout(Carve{}), &sv, &extra, &sort_tmp));
    layout(Carve{extra});
    const int32_t advance = (int32_t)t->advances;
    const bool remove = (t->d.flags & SPH_DUST_REMOVE) != 0;
    dust_kick_drift<<<dim3(blocks(m, KB)), dim3(KB), 0, st>>>(m, t->st, t->smp, t->fates, c->d_dt, t->clk, c->sink, c->sink_radius,
                                                             c->ns, c->p.bounding_size, remove ? 1 : 0, advance, sv.info, pkeys,
                                                             pvals, t->live);
    SPH_HIP(hipGetLastError());
    size_t tmp = psort_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, pkeys, pkeys_alt, pvals, pvals_alt, (size_t)m, 0u, key_bits, st));
    bool row = record;
    if (row && t->rows >= t->d.capacity) { t->dropped++; row = false; }
    double *head = row ? t->head + (size_t)t->rows * NHEAD : nullptr;
    double *body = row ? t->body + (size_t)t->rows * NCOL * (size_t)m : nullptr;
    const DustConst dc{c->p.G, c->p.gamma * c->p.gamma_m1, t->cE, t->d.rho_grain, t->d.law, c->ns, advance};
    const dim3 grid(blocks(m, TB)), block(TB);
    if (per_h) dust_walk<true><<<grid, block, 0, st>>>(pvals_alt, m, sv, h_one, t->st, t->smp, t->fates, t->clk, c->sink, dc, t->live, body);
    else dust_walk<false><<<grid, block, 0, st>>>(pvals_alt, m, sv, h_one, t->st, t->smp, t->fates, t->clk, c->sink, dc, t->live, body);
    dust_head<<<dim3(1), dim3(1), 0, st>>>(c->d_dt, t->clk, t->live, (double)advance, head);
    SPH_HIP(hipGetLastError());
    if (row) t->rows++;
    return SPH_OK;
}

int dust_begin(sph_ctx *c, const sph_dust_desc *d, int64_t n, const double *const *arrays, bool host) {
    const char *who = host ? "sph_dust_begin" : "sph_dust_begin_dev";
    if (!d) return arg_error(c, who, "null descriptor");
    if (n < 1 || n > 0x7fffffffLL) return arg_error(c, who, "the grain count must be 1 .. 2^31 - 1");
    for (int k = 0; k < NST; k++)
        if (!arrays[k]) return arg_error(c, who, "null arrays");
    if (d->capacity < 0) return arg_error(c, who, "capacity must be >= 0");
    if (d->every < 1) return arg_error(c, who, "every must be >= 1");
    if (d->record_every < 1) return arg_error(c, who, "record_every must be >= 1");
    if (d->law != SPH_DUST_EPSTEIN && d->law != SPH_DUST_FIXED_TS) return arg_error(c, who, "unknown law");
    if (d->flags & ~SPH_DUST_REMOVE) return arg_error(c, who, "unknown flags");
    if (d->law == SPH_DUST_EPSTEIN && !(d->rho_grain > 0.0 && std::isfinite(d->rho_grain)))
        return arg_error(c, who, "rho_grain must be > 0 and finite with SPH_DUST_EPSTEIN");
    if (c->nranks > 1 || c->n_owned != c->n) { c->err = std::string(who) + ": one rank and no ghost particles"; return SPH_ERR_STATE; }
    // the drag parameters are checked on the host in both forms: begin may wait
    std::vector<double> par_dev;
    const double *par = arrays[6];
    if (!host) {
        par_dev.resize((size_t)n);
        SPH_HIP(hipMemcpyAsync(par_dev.data(), par, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        SPH_HIP(hipStreamSynchronize(c->stream));
        par = par_dev.data();
    }
    for (int64_t k = 0; k < n; k++)
        if (!(par[k] > 0.0 && std::isfinite(par[k]))) return arg_error(c, who, "a drag parameter is <= 0 or not finite");
    const double body_doubles = (double)d->capacity * (double)NCOL * (double)n;
    if (body_doubles > 1.0e15) { c->err = std::string(who) + ": the log does not fit"; return SPH_ERR_NOMEM; }
    dust_free(c);
    Dust *t = new (std::nothrow) Dust();
    if (!t) { c->err = std::string(who) + ": out of host memory"; return SPH_ERR_NOMEM; }
    c->dust = t;
    t->d = *d;
    t->M = n;
    t->cE = std::sqrt(8.0 / 3.14159265358979323846);
    const size_t body = (size_t)d->capacity * NCOL * (size_t)n;
    int st = ctx_alloc(c, &t->head, (size_t)d->capacity * NHEAD, "dust heads");
    if (st == SPH_OK) st = ctx_alloc(c, &t->body, body, "dust log");
    if (st == SPH_OK) st = ctx_alloc(c, &t->st, (size_t)NST * n, "dust state");
    if (st == SPH_OK) st = ctx_alloc(c, &t->smp, (size_t)NS * n, "dust sample");
    if (st == SPH_OK) st = ctx_alloc(c, &t->clk, 2, "dust clock");
    if (st == SPH_OK) st = ctx_alloc(c, &t->fates, (size_t)3 * n, "dust fates");
    if (st == SPH_OK) st = ctx_alloc(c, &t->live, 1, "dust live count");
    if (st != SPH_OK) { dust_free(c); return st; }
    std::vector<int32_t> f((size_t)3 * n);
    for (int64_t k = 0; k < n; k++) { f[3 * k] = 0; f[3 * k + 1] = 0; f[3 * k + 2] = -1; }
    const int32_t live = (int32_t)n;
    const hipMemcpyKind kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    hipError_t e = body ? hipMemsetAsync(t->body, 0xFF, body * sizeof(double), c->stream) : hipSuccess;   // every byte 0xFF: a NaN
    for (int k = 0; k < NST && e == hipSuccess; k++)
        e = hipMemcpyAsync(t->st + (size_t)k * n, arrays[k], (size_t)n * sizeof(double), kind, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->smp, 0, (size_t)NS * n * sizeof(double), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->fates, f.data(), f.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->live, &live, sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    // the grains' clock starts at the gas clock: the first advance re-samples only
    if (e == hipSuccess) e = hipMemcpyAsync(t->clk, c->d_dt + 1, sizeof(double), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->clk + 1, 0, sizeof(double), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);        // f, live and the host arrays are this call's own
    if (e != hipSuccess) { dust_free(c); SPH_HIP(e); }
    st = dust_run(c, who, false);                                    // the stored sample exists before the first step
    if (st != SPH_OK) dust_free(c);
    return st;
}

int dust_end(sph_ctx *c) {
    if (!c->dust) { c->err = "sph_dust_end: no dust begun"; return SPH_ERR_STATE; }
    dust_free(c);
    return SPH_OK;
}

int dust_advance(sph_ctx *c) {
    Dust *t = c->dust;
    if (!t) { c->err = "sph_dust_advance: no dust begun"; return SPH_ERR_STATE; }
    if (t->closed) { c->err = "sph_dust_advance: the dust is closed (ghosts or several ranks)"; return SPH_ERR_STATE; }
    t->advances++;
    return dust_run(c, "sph_dust_advance", true);
}

int dust_step(sph_ctx *c) {
    Dust *t = c->dust;
    if (!t || t->closed) return SPH_OK;
    t->steps++;
    if (t->steps % t->d.every != 0) return SPH_OK;
    t->advances++;
    t->stepped++;
    return dust_run(c, "sph_step", t->stepped % t->d.record_every == 0);
}

int dust_info(sph_ctx *c, int64_t *rows, int64_t *dropped, int64_t *advances, int64_t *n_grains, int64_t *n_live) {
    const Dust *t = c->dust;
    if (!t) { c->err = "sph_dust_info: no dust begun"; return SPH_ERR_STATE; }
    if (rows) *rows = t->rows;
    if (dropped) *dropped = t->dropped;
    if (advances) *advances = t->advances;
    if (n_grains) *n_grains = t->M;
    if (n_live) {                                        // the one count that lives on the device
        int32_t live = 0;
        SPH_HIP(hipMemcpyAsync(&live, t->live, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        SPH_HIP(hipStreamSynchronize(c->stream));
        *n_live = live;
    }
    return SPH_OK;
}

int dust_read(sph_ctx *c, int64_t first, int64_t count, double *head, double *body, bool host) {
    const char *who = host ? "sph_dust_read" : "sph_dust_read_dev";
    const Dust *t = c->dust;
    if (!t) { c->err = std::string(who) + ": no dust begun"; return SPH_ERR_STATE; }
    if (first < 0 || count < 0 || first > t->rows || count > t->rows - first) return arg_error(c, who, "first / count outside [0, rows]");
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (count > 0 && head)
        SPH_HIP(hipMemcpyAsync(head, t->head + (size_t)first * NHEAD, (size_t)count * NHEAD * sizeof(double), kind, c->stream));
    if (count > 0 && body)
        SPH_HIP(hipMemcpyAsync(body, t->body + (size_t)first * NCOL * (size_t)t->M, (size_t)count * NCOL * (size_t)t->M * sizeof(double),
                               kind, c->stream));
    return SPH_OK;
}

int dust_state(sph_ctx *c, double *const *arrays, bool host) {
    const char *who = host ? "sph_dust_state" : "sph_dust_state_dev";
    const Dust *t = c->dust;
    if (!t) { c->err = std::string(who) + ": no dust begun"; return SPH_ERR_STATE; }
    for (int k = 0; k < NST; k++)
        if (!arrays[k]) return arg_error(c, who, "null output");
    for (int k = 0; k < NST; k++)
        SPH_HIP(hipMemcpyAsync(arrays[k], t->st + (size_t)k * t->M, (size_t)t->M * sizeof(double),
                               host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    return SPH_OK;
}

int dust_fates(sph_ctx *c, int32_t *fates, bool host) {
    const char *who = host ? "sph_dust_fates" : "sph_dust_fates_dev";
    const Dust *t = c->dust;
    if (!t) { c->err = std::string(who) + ": no dust begun"; return SPH_ERR_STATE; }
    if (!fates) return arg_error(c, who, "null output");
    SPH_HIP(hipMemcpyAsync(fates, t->fates, (size_t)3 * (size_t)t->M * sizeof(int32_t), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           c->stream));
    return SPH_OK;
}

}  // namespace sph
