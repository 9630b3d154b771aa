// trace.hip -- field lines of an SPH-interpolated vector field: n_seeds lines of n_steps classical RK4 steps each through the
// frozen field w(q) = sph_sample's normalised value at q, in a frame that may rotate and with the options of
// include/summersph.h (sph_trace).
//
// Not part of the step loop: nothing here reads or writes the context's grid, cell table, neighbour list, statistics or
// flags.  The search structure is sph_sample's, built once per call by sample_build (sample.hip); the walk over it is
// point_sums (sample_common.hpp), so a stage velocity has the bits sph_sample returns at the stage point.
//
// Pipeline (all on ctx->stream):
//   sample_build      select -> levels -> keys -> sort -> records -> tails, with K = 3 rows (4 with a carry)
//   trace_seed_keys + rocprim radix sort   the seeds by their cell in the most populated level (sample_point_keys' rule):
//                     the 64 lanes of a wavefront start in neighbouring cells.  Only the work distribution depends on it.
//   trace_walk<PER_H, CARRY>   one lane per seed: the loop over the steps and the four stages; the stage point, the RK
//                     accumulators and the line's status live in registers; recorded vertices go to the seed's ORIGINAL
//                     index.  A lane whose line has stopped idles until its wavefront is done, then fills its remaining
//                     rows with NaN.  One integer atomic per wavefront and status.
// A line depends only on the sources, the descriptor and its own seed: no float atomics anywhere.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

// the field and the step are written in one documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

#include "sample_common.hpp"

namespace sph {

namespace {

constexpr int KB = 256;                    // block of the seed-key kernel
constexpr int TB = WAVE;                   // block of the walk: one wavefront, so that a long line holds back 63 others at most
constexpr int NSTATUS = 5;
constexpr int RUNNING = -1;

struct TraceParams {
    double box_lo[3], box_hi[3];
    double ds, hs, s6;                     // the step, 0.5 ds and ds / 6
    double om[3], ce[3], nrm[3];           // frame and the unit normal
    int32_t n_steps, stride, n_rec;
    int32_t arclength, planar;
};

__global__ __launch_bounds__(KB) void trace_seed_keys(const double *__restrict__ sx, const double *__restrict__ sy,
                                                      const double *__restrict__ sz, int64_t m, const Info *__restrict__ info,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t t = (int64_t)blockIdx.x * KB + threadIdx.x;
    if (t >= m) return;
    keys[t] = point_sort_key(info, sx[t], sy[t], sz[t]);
    vals[t] = (uint32_t)t;
}

__device__ __forceinline__ bool in_box(const TraceParams &P, const double (&p)[3]) {
    return P.box_lo[0] < p[0] && p[0] < P.box_hi[0] && P.box_lo[1] < p[1] && p[1] < P.box_hi[1] && P.box_lo[2] < p[2] &&
           p[2] < P.box_hi[2];
}

// one lane per seed (the t-th in walk order: seed pidx[t])
template <bool PER_H, bool CARRY>
__global__ __launch_bounds__(TB) void trace_walk(const double *__restrict__ sx, const double *__restrict__ sy,
                                                 const double *__restrict__ sz, const uint32_t *__restrict__ pidx, int64_t m,
                                                 SampleView sv, double h_one, TraceParams P, double *__restrict__ path,
                                                 double *__restrict__ carry_out, int32_t *__restrict__ status,
                                                 int32_t *__restrict__ n_done, unsigned long long *__restrict__ cnt) {
    constexpr int K = CARRY ? 4 : 3;
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    const bool active = t < m;
    const int64_t idx = active ? (int64_t)pidx[t] : 0;
    double p[3] = {0.0, 0.0, 0.0};
    if (active) { p[0] = sx[idx]; p[1] = sy[idx]; p[2] = sz[idx]; }
    const Info *__restrict__ info = sv.info;
    const bool bad = info->bad != 0;
    const int nlev = info->nlev;
    const double ih_one = 1.0 / h_one;                       // one h: the records' 1 / h_j, bitwise
    int code = (bad || !finite3(p[0], p[1], p[2])) ? SPH_TRACE_NONFINITE : RUNNING;
    if (!active) code = SPH_TRACE_DONE;
    int32_t done = 0;                                        // steps taken
    int32_t rows = 0;                                        // recorded vertices so far
    int32_t until = 0;                                       // steps until the next recorded vertex; 0: this one is
    if (code == RUNNING) {
#pragma unroll
        for (int a = 0; a < 3; a++) path[(int64_t)a * m + idx] = p[a];
        rows = 1;
    }
    while (code == RUNNING) {
        const bool rec_here = until == 0;
        const bool inside = in_box(P, p);
        const bool last = !inside || done == P.n_steps;
        const int end_code = inside ? SPH_TRACE_DONE : SPH_TRACE_LEFT_BOX;
        if (last && !(CARRY && rec_here)) { code = end_code; break; }
        double q[3] = {p[0], p[1], p[2]};
        double A[3] = {0.0, 0.0, 0.0}, B[3] = {0.0, 0.0, 0.0};
        int stop = RUNNING;
#pragma unroll 1
        for (int stg = 0; stg < 4; stg++) {
            double den = 0.0, num[K];
#pragma unroll
            for (int k = 0; k < K; k++) num[k] = 0.0;
            point_sums<K, PER_H>(info, sv.rec, sv.wsa, sv.tab, sv.mask, nlev, q, ih_one, den, num);
            if (stg == 0) {
                if (CARRY && rec_here) carry_out[(int64_t)(rows - 1) * m + idx] = den != 0.0 ? num[K - 1] / den : 0.0;
                if (last) { stop = end_code; break; }
            }
            if (den == 0.0) { stop = SPH_TRACE_LEFT_GAS; break; }
            double v[3];
            {
                const double w0 = num[0] / den, w1 = num[1] / den, w2 = num[2] / den;
                const double t0 = q[0] - P.ce[0], t1 = q[1] - P.ce[1], t2 = q[2] - P.ce[2];
                const double f0 = P.om[1] * t2 - P.om[2] * t1;
                const double f1 = P.om[2] * t0 - P.om[0] * t2;
                const double f2 = P.om[0] * t1 - P.om[1] * t0;
                v[0] = w0 - f0; v[1] = w1 - f1; v[2] = w2 - f2;
            }
            if (P.planar) {
                const double d = (v[0] * P.nrm[0] + v[1] * P.nrm[1]) + v[2] * P.nrm[2];
#pragma unroll
                for (int a = 0; a < 3; a++) v[a] = v[a] - d * P.nrm[a];
            }
            if (P.arclength) {
                const double sp = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
                if (!(sp > 0.0 && sp <= SAMPLE_DBL_BIG)) { stop = SPH_TRACE_STAGNANT; break; }
#pragma unroll
                for (int a = 0; a < 3; a++) v[a] = v[a] / sp;
            }
            // (k1 + 2 k2) in A, (2 k3 + k4) in B; the next stage point
            const double c = stg == 2 ? P.ds : P.hs;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (stg < 2) A[a] = stg == 0 ? v[a] : A[a] + 2.0 * v[a];
                else B[a] = stg == 2 ? 2.0 * v[a] : B[a] + v[a];
                if (stg < 3) q[a] = p[a] + c * v[a];
            }
        }
        if (stop != RUNNING) { code = stop; break; }
#pragma unroll
        for (int a = 0; a < 3; a++) p[a] = p[a] + P.s6 * (A[a] + B[a]);
        done++;
        until = (until == 0 ? P.stride : until) - 1;
        if (until == 0) {
#pragma unroll
            for (int a = 0; a < 3; a++) path[((int64_t)rows * 3 + a) * m + idx] = p[a];
            rows++;
        }
    }
    if (active) {
        for (int32_t r = rows; r <= P.n_rec; r++) {
#pragma unroll
            for (int a = 0; a < 3; a++) path[((int64_t)r * 3 + a) * m + idx] = NAN;
            if (CARRY) carry_out[(int64_t)r * m + idx] = NAN;
        }
        status[idx] = code;
        n_done[idx] = done;
    }
    // counts: one integer atomic per wavefront and status; a bad source h shows as cnt[0] == -1 and nothing else
    if (bad) {
        if (t == 0) cnt[0] = ~0ull;
        return;
    }
#pragma unroll
    for (int s = 0; s < NSTATUS; s++) {
        const unsigned long long hit = __ballot(active && code == s);
        if ((threadIdx.x & (WAVE - 1)) == 0 && hit) atomicAdd(&cnt[s], (unsigned long long)__popcll(hit));
    }
}

struct WalkArgs {
    const double *sx, *sy, *sz;
    const uint32_t *pidx;
    int64_t m;
    SampleView sv;
    double h_one;
    TraceParams P;
    double *path, *carry;
    int32_t *status, *n_done;
    unsigned long long *cnt;
};

template <bool PER_H, bool CARRY>
hipError_t launch_walk(hipStream_t st, const WalkArgs &a) {
    trace_walk<PER_H, CARRY><<<dim3(blocks(a.m, TB)), dim3(TB), 0, st>>>(a.sx, a.sy, a.sz, a.pidx, a.m, a.sv, a.h_one, a.P, a.path,
                                                                         a.carry, a.status, a.n_done, a.cnt);
    return hipGetLastError();
}

bool finite_all(const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

bool field_id_ok(int32_t f) { return f == SPH_TRACE_VALUES || (f >= 0 && f < SPH_F_COUNT); }

}  // namespace

int trace_run(sph_ctx *c, const sph_trace_desc *d, int64_t n_seeds, const double *sx, const double *sy, const double *sz,
              const double *values, double *path, int64_t n_path, double *carry_out, int32_t *status, int32_t *n_done,
              int64_t *counts, bool host) {
    const char *who = "sph_trace";
    if (!d) return arg_error(c, who, "null descriptor");
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return arg_error(c, who, "reserved must be 0");
    if (d->flags & ~(SPH_TRACE_ARCLENGTH | SPH_TRACE_PLANAR)) return arg_error(c, who, "unknown flags");
    if (n_seeds < 0 || n_seeds > 0x7fffffffLL) return arg_error(c, who, "n_seeds must be 0 .. 2^31 - 1");
    if (n_seeds > 0 && (!sx || !sy || !sz)) return arg_error(c, who, "null seed arrays");
    if (!std::isfinite(d->ds) || d->ds == 0.0) return arg_error(c, who, "ds must be finite and != 0");
    if (d->n_steps < 1 || d->n_steps > 65535) return arg_error(c, who, "n_steps must be 1 .. 65535");
    if (d->stride < 1 || d->n_steps % d->stride != 0) return arg_error(c, who, "stride must be >= 1 and divide n_steps");
    const bool carry = d->carry != SPH_TRACE_NONE;
    bool any_values = carry && d->carry == SPH_TRACE_VALUES;
    for (int k = 0; k < 3; k++) {
        if (!field_id_ok(d->fields[k])) return arg_error(c, who, "field id out of range");
        any_values = any_values || d->fields[k] == SPH_TRACE_VALUES;
    }
    if (carry && !field_id_ok(d->carry)) return arg_error(c, who, "carry id out of range");
    if (any_values != (values != nullptr)) return arg_error(c, who, "values must be given with SPH_TRACE_VALUES and only then");
    const int64_t n_rec = d->n_steps / d->stride;
    if (n_path != 3 * (n_rec + 1) * n_seeds) return arg_error(c, who, "n_path != 3 (n_rec + 1) n_seeds");
    if (!path || !status || !n_done) return arg_error(c, who, "null path, status or n_done");
    if (carry != (carry_out != nullptr)) return arg_error(c, who, "carry_out must be given with a carry and only then");
    const bool planar = (d->flags & SPH_TRACE_PLANAR) != 0;
    if (planar && (!finite_all(d->normal) || (d->normal[0] == 0.0 && d->normal[1] == 0.0 && d->normal[2] == 0.0)))
        return arg_error(c, who, "SPH_TRACE_PLANAR needs a finite non-zero normal");
    if (!finite_all(d->omega) || !finite_all(d->centre)) return arg_error(c, who, "omega and centre must be finite");
    for (int a = 0; a < 3; a++)
        if (std::isnan(d->clip_lo[a]) || std::isnan(d->clip_hi[a]) || std::isnan(d->box_lo[a]) || std::isnan(d->box_hi[a]))
            return arg_error(c, who, "a box has a NaN");
    if (std::isnan(d->h) || d->h < 0.0) return arg_error(c, who, "h must be >= 0");
    if (d->weight != SPH_RENDER_WEIGHT_MASS && d->weight != SPH_RENDER_WEIGHT_VOLUME) return arg_error(c, who, "unknown weight");
    TraceParams P{};
    if (planar) {
        const double len = std::sqrt((d->normal[0] * d->normal[0] + d->normal[1] * d->normal[1]) + d->normal[2] * d->normal[2]);
        if (!(len > 0.0) || !std::isfinite(len)) return arg_error(c, who, "the normal's length underflows or overflows");
        for (int a = 0; a < 3; a++) P.nrm[a] = d->normal[a] / len;
    }
    const bool volume = d->weight == SPH_RENDER_WEIGHT_VOLUME;
    const int nf = carry ? 4 : 3;
    const int32_t fields[4] = {d->fields[0], d->fields[1], d->fields[2], carry ? d->carry : 0};
    bool stale = volume && !field_ready(*c, c->variable, SPH_F_RHO);
    for (int k = 0; k < nf; k++) stale = stale || (fields[k] >= 0 && !field_ready(*c, c->variable, fields[k]));
    if (stale) {
        c->err = "sph_trace: a field or rho is stale (sph_download_field would refuse it)";
        return SPH_ERR_STATE;
    }
    const bool per_h = !(d->h > 0.0) && c->variable;
    const double h_one = d->h > 0.0 ? d->h : (c->variable ? 0.0 : c->p.h);
    if (!per_h && !(h_one > 0.0)) {
        c->err = "sph_trace: params.h <= 0 on a fixed-h context (give desc.h > 0)";
        return SPH_ERR_STATE;
    }
    if (n_seeds == 0) {
        if (host) {
            if (counts) std::memset(counts, 0, NSTATUS * sizeof(int64_t));
        } else if (counts) {
            SPH_HIP(hipMemsetAsync(counts, 0, NSTATUS * sizeof(int64_t), c->stream));
        }
        return SPH_OK;
    }
    for (int a = 0; a < 3; a++) {
        P.box_lo[a] = d->box_lo[a]; P.box_hi[a] = d->box_hi[a];
        P.om[a] = d->omega[a]; P.ce[a] = d->centre[a];
    }
    P.ds = d->ds;
    P.hs = 0.5 * d->ds;
    P.s6 = d->ds / 6.0;
    P.n_steps = d->n_steps; P.stride = d->stride; P.n_rec = (int32_t)n_rec;
    P.arclength = (d->flags & SPH_TRACE_ARCLENGTH) ? 1 : 0;
    P.planar = planar ? 1 : 0;

    hipStream_t st = c->stream;
    const int64_t m = n_seeds;
    const size_t n_carry = carry ? (size_t)(n_rec + 1) * (size_t)m : 0;
    size_t psort_bytes = 0;
    SPH_HIP(rocprim::radix_sort_pairs(nullptr, psort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)m, 0u, (unsigned)(3 * LEVEL_AXIS_BITS + 1), st));
    uint64_t *pkeys, *pkeys_alt;
    uint32_t *pvals, *pvals_alt;
    unsigned long long *cnt;
    double *h_seeds, *h_path, *h_carry;
    int32_t *h_status, *h_done;
    auto layout = [&](Carve cv) {
        pkeys = cv.take<uint64_t>(m);
        pkeys_alt = cv.take<uint64_t>(m);
        pvals = cv.take<uint32_t>(m);
        pvals_alt = cv.take<uint32_t>(m);
        cnt = cv.take<unsigned long long>(NSTATUS);
        h_seeds = cv.take<double>(host ? 3 * (size_t)m : 0);    // the host form's device copies
        h_path = cv.take<double>(host ? n_path : 0);
        h_carry = cv.take<double>(host ? n_carry : 0);
        h_status = cv.take<int32_t>(host ? m : 0);
        h_done = cv.take<int32_t>(host ? m : 0);
        return cv.bytes;
    };
    const SampleSources src{d->clip_lo, d->clip_hi, h_one, per_h, volume, host, nf, fields, values, psort_bytes};
    SampleView sv{};
    char *extra = nullptr, *sort_tmp = nullptr;
    SPH_TRY(sample_build(c, src, layout(Carve{}), &sv, &extra, &sort_tmp));
    layout(Carve{extra});
    const double *d_sx = sx, *d_sy = sy, *d_sz = sz;
    if (host) {
        SPH_TRY(analysis_pinned(c));
        SPH_HIP(hipMemcpyAsync(h_seeds, sx, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        SPH_HIP(hipMemcpyAsync(h_seeds + m, sy, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        SPH_HIP(hipMemcpyAsync(h_seeds + 2 * m, sz, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        d_sx = h_seeds; d_sy = h_seeds + m; d_sz = h_seeds + 2 * m;
    }
    // the seeds in the order of their cells
    trace_seed_keys<<<dim3(blocks(m, KB)), dim3(KB), 0, st>>>(d_sx, d_sy, d_sz, m, sv.info, pkeys, pvals);
    SPH_HIP(hipGetLastError());
    size_t tmp = psort_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, pkeys, pkeys_alt, pvals, pvals_alt, (size_t)m, 0u,
                                      (unsigned)(3 * LEVEL_AXIS_BITS + 1), st));
    SPH_HIP(hipMemsetAsync(cnt, 0, NSTATUS * sizeof(unsigned long long), st));
    const WalkArgs wa{d_sx, d_sy, d_sz, pvals_alt, m, sv, h_one, P, host ? h_path : path, host ? (carry ? h_carry : nullptr) : carry_out,
                      host ? h_status : status, host ? h_done : n_done, cnt};
    hipError_t e = hipSuccess;
    if (per_h) e = carry ? launch_walk<true, true>(st, wa) : launch_walk<true, false>(st, wa);
    else e = carry ? launch_walk<false, true>(st, wa) : launch_walk<false, false>(st, wa);
    SPH_HIP(e);
    if (!host) {
        if (counts) SPH_HIP(hipMemcpyAsync(counts, cnt, NSTATUS * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        return SPH_OK;
    }
    // host form: the counts first (a bad source h writes nothing to the caller), then the rows in one read-back
    SPH_HIP(hipMemcpyAsync(c->rnd_pinned, cnt, NSTATUS * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipMemcpyAsync(path, h_path, (size_t)n_path * sizeof(double), hipMemcpyDeviceToHost, st));
    if (carry) SPH_HIP(hipMemcpyAsync(carry_out, h_carry, n_carry * sizeof(double), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipMemcpyAsync(status, h_status, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipMemcpyAsync(n_done, h_done, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    int64_t cc[NSTATUS];
    std::memcpy(cc, c->rnd_pinned, sizeof(cc));
    if (cc[0] < 0) {
        c->err = "sph_trace: a selected particle has h <= 0 or a non-finite h";
        return SPH_ERR_STATE;
    }
    if (counts) std::memcpy(counts, cc, sizeof(cc));
    return SPH_OK;
}

}  // namespace sph
