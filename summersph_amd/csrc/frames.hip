// frames.hip -- the movie of a run (include/summersph.h, sph_frames): a device-resident log of line-of-sight-integrated
// maps of the owned gas, one row of (1 + nq) n_u n_v doubles and a head of 16 per recorded step, appended from the end of
// the step by kernels on the context's stream, and the one-shot sph_frame, which is the same kernels on the analysis
// scratch.  Frame, selection, h rule and nodes are sph_cube's (image_common.hpp), the footprint is spline_column.hpp.
//
// Only reads the context: the state, the grid, the list, the statistics, dt and every validity flag stay as they are, and
// with no frames begun the step enqueues exactly what it enqueued before.
//
// A node's sum is exact (exact_sum.hpp): every term y0 A F(p) is rounded half-even to a multiple of 2^(e - 62), with 2^e
// above 1.5 max |y0 A| of its plane, and added in 128-bit integers; a node is converted once.  The image therefore does
// not depend on the order of the adds: no sort, no list, no capacity, nothing the host has to size -- which is what lets a
// frame be enqueued behind a step.  The passes run over the sorted slots, whose order changes at every grid build.
//
// Whether a frame is due, its row and the dropped count are device words (Ctl).  Five launches per frame, all on
// ctx->stream; with dt_frame > 0 they are enqueued every step and return at once where no frame is due:
//   frames_maxima   every slot: per-block max |y0 A| of each plane, the non-finite marks, the selected count
//   frames_head     one block: the partials -> exponents and marks; the centre (the sink's position now); the due decision,
//                   the row and the cadence counter
//   frames_clear    the limb image -> 0
//   frames_splat    a block per run of SB consecutive sorted slots (spatially compact), no grid stride: what the setup of a
//                   run needs (selection, frame, clip) is dead before the pair loop, which keeps the kernel inside the
//                   scalar registers.  The run's (particle, node) pairs are numbered across the block so that F -- four
//                   logarithms, half a dozen square roots -- is evaluated at full lane occupancy whatever a particle
//                   covers; a pair inside the run's LDS window of limbs is added there (LDS atomics), a pair outside it
//                   straight to the global limbs; the window's non-zero limbs are flushed row-contiguously
//   frames_finish   limbs -> doubles into the row, and the head
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "exact_sum.hpp"
#include "image_common.hpp"
#include "spline_column.hpp"

// every term in the documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int NP = 1 + SPH_FRAMES_MAX_FIELDS;  // planes at most
constexpr int NHEAD = SPH_FRAMES_NHEAD;
constexpr int MB = 256;                        // block of the maxima pass
constexpr int M_BLOCKS = 1024;                 // its blocks at most (grid-stride beyond)
constexpr int SB = 256;                        // block of the splat = slots of a run
constexpr int NMX = NP + 1;                    // maxima: the planes' max |y0 A|, then the selected count (a sum)
constexpr int64_t MAX_NODES = (int64_t)1 << 28;   // (1 + nq) n_u n_v at most: a particle's pair count stays an int32

// the device words of a log (or of a one-shot call)
struct Ctl {
    long long rows, dropped, k;                // rows held, frames dropped, the next threshold is t0 + k dt_frame
    long long n_sel;                           // selected particles of the frame in hand
    double t0;                                 // the context's t at begin
    double centre[3];                          // the centre of the frame in hand
    int32_t exps[NP];
    uint32_t bad;                              // bit q: plane q has a non-finite term (or its field is not current)
    int32_t due, status;                       // the frame in hand: is written; SPH_FRAMES_OK / _SINK_GONE
    long long row;                             // its row
};

struct Args {
    Sel sel;
    Frame fr;                                  // centre: the descriptor's; the sink's position is added in frames_head
    Nodes<2> nd;
    const double *x, *y, *z, *m;
    const double *A[SPH_FRAMES_MAX_FIELDS];    // sorted order; null: sph_download_field would refuse the field now
    const double *sink, *d_dt;
    Ctl *ctl;
    double *part;                              // frames_maxima's partials: M_BLOCKS x NMX
    uint32_t *bad_part;
    unsigned long long *limbs;                 // [plane][lo, hi][node]
    double *heads, *planes;                    // the log (or the one-shot call's outputs)
    double dt_frame, step, n_gas;
    long long capacity;
    int32_t nq, centre_sink, ns, force;        // force: this frame is due whatever t says (every-k cadence, record, one-shot)
    int32_t win;                               // the splat's LDS window: win x win nodes (0: none)
};

// t has reached the next threshold (product, then sum, in double)
__device__ __forceinline__ bool threshold_passed(const Args &a) {
    return a.dt_frame > 0.0 && a.d_dt[1] >= a.ctl->t0 + (double)a.ctl->k * a.dt_frame;
}

// y0 = m / (pi h^2) (sph_transfer's expression with kappa = 1) times A per plane
__device__ __forceinline__ void weights(const Args &a, int64_t i, double h, double (&w)[NP]) {
    const double y0 = a.m[i] / (M_PI * (h * h));
    w[0] = y0;
#pragma unroll
    for (int q = 1; q < NP; q++) w[q] = (q <= a.nq && a.A[q - 1]) ? y0 * a.A[q - 1][i] : 0.0;
}

__global__ __launch_bounds__(MB) void frames_maxima(Args a) {
    __shared__ uint32_t s_bad[MB / WAVE];
    if (!(a.force || threshold_passed(a)) || a.ctl->rows >= a.capacity) return;      // frames_head decides the same
    double v[NMX];
#pragma unroll
    for (int q = 0; q < NP; q++) v[q] = -INFINITY;
    v[NP] = 0.0;
    uint32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x; i < a.sel.n_slots; i += (int64_t)gridDim.x * MB) {
        if (a.sel.orig[i] < 0 || !selected(a.sel, i, a.x[i], a.y[i], a.z[i])) continue;
        double w[NP];
        weights(a, i, sel_h(a.sel, i), w);
#pragma unroll
        for (int q = 0; q < NP; q++) {
            v[q] = fmax(v[q], fabs(w[q]));
            if (!finite(1.5 * w[q])) bad |= 1u << q;
        }
        v[NP] += 1.0;
    }
    bad = wave_or(bad);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) s_bad[wv] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MB / WAVE; w++) bad |= s_bad[w];
        a.bad_part[blockIdx.x] = bad;
    }
    stats_block_partial<0, NP, MB, NMX>(v, a.part);
}

// One block of NMX wavefronts: wave q < NP joins the maximum and the marks of plane q, wave NP the selected count and
// everything that is decided once per frame.  The waves write disjoint words of Ctl and read none that another writes.
__global__ __launch_bounds__(NMX * WAVE) void frames_head(Args a, int nb) {
    Ctl *c = a.ctl;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const bool passed = threshold_passed(a);
    const bool due = (a.force || passed) && c->rows < a.capacity;
    double v = q < NP ? -INFINITY : 0.0;
    uint32_t bad = 0;
    if (due)
        for (int b = lane; b < nb; b += WAVE) {
            v = stat_join<0, NP>(q, v, a.part[b * NMX + q]);
            bad |= a.bad_part[b];
        }
    v = stat_wave<0, NP>(q, v);
    bad = wave_or(bad);
    __syncthreads();                                       // every wave has read rows, k and t0
    if (lane != 0) return;
    if (q < NP) {
        for (int k = 1; k <= a.nq; k++)
            if (!a.A[k - 1]) bad |= 1u << k;               // the field is not current: its plane is NaN
        c->exps[q] = (bad >> q & 1u) ? 0 : exp_above(1.5 * fmax(v, 0.0));
        if (q == 0) c->bad = bad;                          // the marks of all planes came with every partial
        return;
    }
    c->n_sel = (long long)v;
    int32_t status = SPH_FRAMES_OK;
    double ctr[3] = {a.fr.centre[0], a.fr.centre[1], a.fr.centre[2]};
    if (a.centre_sink >= 0) {
        if (a.centre_sink < a.ns) {
#pragma unroll
            for (int k = 0; k < 3; k++) ctr[k] = ctr[k] + a.sink[k * MAX_SINKS + a.centre_sink];
        } else {
            status = SPH_FRAMES_SINK_GONE;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) c->centre[k] = ctr[k];
    c->status = status;
    c->due = due ? 1 : 0;
    c->row = c->rows;
    if ((a.force || passed) && !due) c->dropped++;
    if (due) c->rows++;
    if (!a.force && passed) c->k = (long long)floor((a.d_dt[1] - c->t0) / a.dt_frame) + 1;
}

__global__ __launch_bounds__(256) void frames_clear(const Ctl *__restrict__ ctl, unsigned long long *__restrict__ limbs, int64_t n) {
    if (!ctl->due) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) limbs[i] = 0ull;
}

// WIN: with the LDS window.  Dynamic LDS: 2 nplanes win^2 words
template <bool WIN>
__global__ __launch_bounds__(SB) void frames_splat(Args a) {
    extern __shared__ unsigned long long s_win[];          // [plane][lo, hi][wu][wv]
    __shared__ double s_pu[SB], s_pv[SB], s_h[SB], s_w[NP][SB];
    __shared__ int32_t s_u0[SB], s_v0[SB], s_nv[SB];
    __shared__ unsigned long long s_end[SB];               // inclusive scan of the particles' pair counts
    __shared__ int32_t s_lo[2][SB / WAVE];
    const Ctl *c = a.ctl;
    if (!c->due || c->status != SPH_FRAMES_OK) return;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const Nodes<2> &nd = a.nd;
    const int np = 1 + a.nq;
    const int64_t pixels = (int64_t)nd.n[0] * nd.n[1];
    const uint32_t bad = c->bad;
    int sh[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) sh[q] = 62 - c->exps[q];
    const double c0 = c->centre[0], c1 = c->centre[1], c2 = c->centre[2];
    const int W = WIN ? a.win : 0, wsz = W * W;

    {
        const int64_t i = (int64_t)blockIdx.x * SB + t;
        int cnt = 0, u0 = 0, v0 = 0, nu = 0, nv = 0;
        if (i < a.sel.n_slots && a.sel.orig[i] >= 0 && selected(a.sel, i, a.x[i], a.y[i], a.z[i])) {
            const double h = sel_h(a.sel, i);
            const double dx = a.x[i] - c0, dy = a.y[i] - c1, dz = a.z[i] - c2;
            const double pu = row_dot(a.fr.rot, 0, dx, dy, dz), pv = row_dot(a.fr.rot, 1, dx, dy, dz);
            const double reach = reach_of(h);
            int u1, v1;
            if (node_range(nd, 0, pu, reach, u0, u1) && node_range(nd, 1, pv, reach, v0, v1)) {
                nu = u1 - u0 + 1;
                nv = v1 - v0 + 1;
                cnt = nu * nv;                             // <= n_u n_v <= MAX_NODES
                double w[NP];
                weights(a, i, h, w);
                s_pu[t] = pu; s_pv[t] = pv; s_h[t] = h;
#pragma unroll
                for (int q = 0; q < NP; q++) s_w[q][t] = w[q];
            }
        }
        s_u0[t] = u0; s_v0[t] = v0; s_nv[t] = nv;
        s_end[t] = (unsigned long long)cnt;
        // the window's corner: the lowest first node of the run's particles on each axis
        int mu = cnt ? u0 : 0x7fffffff, mv = cnt ? v0 : 0x7fffffff;
        if (WIN) {
            for (int o = 32; o > 0; o >>= 1) { mu = min(mu, __shfl_xor(mu, o, 64)); mv = min(mv, __shfl_xor(mv, o, 64)); }
            if (lane == 0) { s_lo[0][wv] = mu; s_lo[1][wv] = mv; }
            for (int k = t; k < 2 * np * wsz; k += SB) s_win[k] = 0ull;
        }
        __syncthreads();
        for (int o = 1; o < SB; o <<= 1) {                 // inclusive scan
            const unsigned long long add = t >= o ? s_end[t - o] : 0ull;
            __syncthreads();
            s_end[t] += add;
            __syncthreads();
        }
        const unsigned long long total = s_end[SB - 1];
        if (WIN) {
            mu = s_lo[0][0]; mv = s_lo[1][0];
            for (int w = 1; w < SB / WAVE; w++) { mu = min(mu, s_lo[0][w]); mv = min(mv, s_lo[1][w]); }
        }
        for (unsigned long long q0 = t; q0 < total; q0 += SB) {
            int lo = 0, hi = SB - 1;                       // the first particle whose scan exceeds q0
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_end[mid] > q0) hi = mid; else lo = mid + 1;
            }
            const int j = lo;
            const int r = (int)(q0 - (j ? s_end[j - 1] : 0ull));
            const int pnv = s_nv[j];
            const int iu = s_u0[j] + r / pnv, iv = s_v0[j] + r % pnv;
            const double du = node_coord(nd, 0, iu) - s_pu[j], dv = node_coord(nd, 1, iv) - s_pv[j];
            const double p = sqrt(du * du + dv * dv) / s_h[j];
            if (!(p < 2.0)) continue;
            const double F = spline_column(p);
            const int64_t node = (int64_t)iu * nd.n[1] + iv;
            const int wu = iu - mu, wvv = iv - mv;
            const bool inside = WIN && wu < W && wvv < W;  // wu, wvv >= 0: the corner is the minimum
#pragma unroll
            for (int pl = 0; pl < NP; pl++) {
                if (pl >= np || (bad >> pl & 1u)) continue;
                const long long f = to_fixed(s_w[pl][j] * F, sh[pl]);
                if (f == 0) continue;
                const unsigned long long tu = (unsigned long long)f, sign = (unsigned long long)(f >> 63);
                if (inside) {
                    unsigned long long *wl = s_win + (size_t)(2 * pl) * wsz + wu * W + wvv;
                    add_limbs_shared(wl, wl + wsz, tu, sign);
                } else {
                    unsigned long long *gl = a.limbs + (size_t)(2 * pl) * pixels + node;
                    add_limbs_shared(gl, gl + pixels, tu, sign);
                }
            }
        }
        __syncthreads();
        if (WIN) {
            // the flush: consecutive lanes take consecutive nodes of a window row
            for (int k = t; k < np * wsz; k += SB) {
                const int pl = k / wsz, rem = k % wsz;
                const int iu = mu + rem / W, iv = mv + rem % W;
                const unsigned long long l = s_win[(size_t)(2 * pl) * wsz + rem], h = s_win[(size_t)(2 * pl + 1) * wsz + rem];
                if ((l | h) == 0ull) continue;             // only nodes inside the image were added to
                unsigned long long *gl = a.limbs + (size_t)(2 * pl) * pixels + ((int64_t)iu * nd.n[1] + iv);
                add_limbs_shared(gl, gl + pixels, l, h);
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void frames_finish(Args a) {
    const Ctl *c = a.ctl;
    if (!c->due) return;
    const int np = 1 + a.nq;
    const int64_t pixels = (int64_t)a.nd.n[0] * a.nd.n[1];
    double *out = a.planes + (size_t)c->row * (size_t)np * (size_t)pixels;
    const bool gone = c->status != SPH_FRAMES_OK;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < np * pixels; i += (int64_t)gridDim.x * 256) {
        const int pl = (int)(i / pixels);
        const int64_t node = i % pixels;
        double v = NAN;
        if (!gone && !(c->bad >> pl & 1u))
            v = limbs_to_double(a.limbs[(size_t)(2 * pl) * pixels + node], a.limbs[(size_t)(2 * pl + 1) * pixels + node], c->exps[pl]);
        out[i] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < NHEAD) {
        const int k = threadIdx.x;
        double v = 0.0;
        if (k == 0) v = a.step;
        else if (k == 1) v = a.d_dt[1];
        else if (k == 2) v = a.n_gas;
        else if (k == 3) v = (double)c->n_sel;
        else if (k < 7) v = c->centre[k - 4];
        else if (k < 7 + NP) v = (k - 7 < np && !(c->bad >> (k - 7) & 1u)) ? (double)c->exps[k - 7] : (double)NAN;
        else if (k == 7 + NP) v = (double)c->status;
        a.heads[(size_t)c->row * NHEAD + k] = v;
    }
}

// the splat's form: SPH_FRAMES_SPLAT=plain takes every pair straight to the global limbs (the form the window is measured
// against); the result is the same bit for bit
bool splat_plain() { return switches().frames_splat_plain; }

int check_desc(sph_ctx *c, const char *who, const sph_frames_desc *d, bool log) {
    if (!d) return arg_error(c, who, "null descriptor");
    if (d->reserved != 0) return arg_error(c, who, "reserved must be 0");
    if (d->n_u < 1 || d->n_v < 1) return arg_error(c, who, "n_u and n_v must be >= 1");
    if (d->nq < 0 || d->nq > SPH_FRAMES_MAX_FIELDS) return arg_error(c, who, "nq must be 0 .. 3");
    for (int k = 0; k < d->nq; k++)
        if (d->fields[k] < 0 || d->fields[k] >= SPH_F_COUNT) return arg_error(c, who, "unknown field id");
    if (!(d->h >= 0.0) || !std::isfinite(d->h)) return arg_error(c, who, "h must be finite and >= 0");
    for (int a = 0; a < 2; a++)
        if (!(d->lo[a] <= d->hi[a]) || !std::isfinite(d->lo[a]) || !std::isfinite(d->hi[a])) return arg_error(c, who, "lo > hi");
    for (int a = 0; a < 3; a++) {
        if (std::isnan(d->clip_lo[a]) || std::isnan(d->clip_hi[a])) return arg_error(c, who, "NaN clip box");
        if (!std::isfinite(d->centre[a])) return arg_error(c, who, "centre must be finite");
    }
    if (!check_rot(d->rot)) return arg_error(c, who, "rot must be orthonormal and right-handed within 1e-12");
    if (d->centre_sink >= MAX_SINKS) return arg_error(c, who, "centre_sink must be < 64 (negative: none)");
    if (log) {
        if (d->capacity < 1) return arg_error(c, who, "capacity must be >= 1");
        const bool by_step = d->every >= 1, by_time = d->dt_frame > 0.0;
        if (std::isnan(d->dt_frame) || d->dt_frame < 0.0 || std::isinf(d->dt_frame) || d->every < 0)
            return arg_error(c, who, "every must be >= 0 and dt_frame finite and >= 0");
        if (by_step == by_time) return arg_error(c, who, "exactly one cadence: every >= 1 with dt_frame == 0, or dt_frame > 0 with every == 0");
    }
    if ((int64_t)d->n_u * d->n_v > MAX_NODES / (1 + d->nq)) { c->err = std::string(who) + ": the image does not fit"; return SPH_ERR_NOMEM; }
    return SPH_OK;
}

// what a frame needs besides the descriptor
struct Work {
    Ctl *ctl;
    double *part;
    uint32_t *bad_part;
    unsigned long long *limbs;
};

size_t limb_words(const sph_frames_desc &d) { return (size_t)2 * (1 + d.nq) * (size_t)d.n_u * (size_t)d.n_v; }

// enqueues the five launches of one frame of the state as it is now
int enqueue(sph_ctx *c, const sph_frames_desc &d, const Work &w, double *heads, double *planes, long long capacity, bool force,
            double step) {
    Args a{};
    a.sel = make_sel(c, d.clip_lo, d.clip_hi, d.h);
    std::memcpy(a.fr.rot, d.rot, sizeof a.fr.rot);
    std::memcpy(a.fr.centre, d.centre, sizeof a.fr.centre);
    const double lo[2] = {d.lo[0], d.lo[1]}, hi[2] = {d.hi[0], d.hi[1]};
    const int32_t n[2] = {d.n_u, d.n_v};
    a.nd = make_nodes<2>(lo, hi, n);
    a.x = c->f[SPH_F_X]; a.y = c->f[SPH_F_Y]; a.z = c->f[SPH_F_Z]; a.m = c->f[SPH_F_M];
    for (int k = 0; k < d.nq; k++)
        a.A[k] = (a.sel.n_slots > 0 && field_ready(*c, c->variable, d.fields[k])) ? c->f[d.fields[k]] : nullptr;
    a.sink = c->sink; a.d_dt = c->d_dt;
    a.ctl = w.ctl; a.part = w.part; a.bad_part = w.bad_part; a.limbs = w.limbs;
    a.heads = heads; a.planes = planes;
    a.dt_frame = d.dt_frame; a.step = step; a.n_gas = (double)(a.sel.n_slots > 0 ? c->n_owned : 0);
    a.capacity = capacity;
    a.nq = d.nq; a.centre_sink = d.centre_sink; a.ns = c->ns; a.force = force ? 1 : 0;
    a.win = splat_plain() ? 0 : (1 + d.nq <= 2 ? 32 : 16);
    hipStream_t st = c->stream;
    const int nb = (int)std::min<int64_t>(blocks(a.sel.n_slots, MB), M_BLOCKS);
    const int64_t n_runs = (a.sel.n_slots + SB - 1) / SB;
    const int64_t words = (int64_t)limb_words(d);
    frames_maxima<<<dim3((unsigned)nb), dim3(MB), 0, st>>>(a);
    frames_head<<<dim3(1), dim3(NMX * WAVE), 0, st>>>(a, nb);
    frames_clear<<<dim3(std::min<unsigned>(blocks(words, 256 * 4), 2048)), dim3(256), 0, st>>>(w.ctl, w.limbs, words);
    if (n_runs > 0) {
        const unsigned sb = (unsigned)n_runs;                 // n_slots < 2^31
        if (a.win) frames_splat<true><<<dim3(sb), dim3(SB), (size_t)2 * (1 + d.nq) * a.win * a.win * sizeof(unsigned long long), st>>>(a);
        else frames_splat<false><<<dim3(sb), dim3(SB), 0, st>>>(a);
    }
    frames_finish<<<dim3(std::min<unsigned>(blocks(words / 2, 256), 2048)), dim3(256), 0, st>>>(a);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

__global__ void frames_init(Ctl *ctl, const double *__restrict__ d_dt) {
    Ctl z{};
    z.k = 1;
    z.t0 = d_dt[1];
    *ctl = z;
}

}  // namespace

struct Frames {
    sph_frames_desc d{};
    int64_t steps = 0;
    double *heads = nullptr, *planes = nullptr;            // capacity x NHEAD, capacity x (1 + nq) n_u n_v
    Work w{};
};

void frames_free(sph_ctx *c) {
    Frames *f = c->frames;
    if (!f) return;
    ctx_free(c, f->heads); ctx_free(c, f->planes); ctx_free(c, f->w.ctl); ctx_free(c, f->w.part); ctx_free(c, f->w.bad_part);
    ctx_free(c, f->w.limbs);
    delete f;
    c->frames = nullptr;
}

int frames_begin(sph_ctx *c, const sph_frames_desc *d) {
    const char *who = "sph_frames_begin";
    SPH_TRY(check_desc(c, who, d, true));
    const size_t row = limb_words(*d) / 2;
    if ((double)d->capacity * (double)row > 1.0e15) { c->err = std::string(who) + ": the log does not fit"; return SPH_ERR_NOMEM; }
    frames_free(c);
    Frames *f = new (std::nothrow) Frames();
    if (!f) { c->err = std::string(who) + ": out of host memory"; return SPH_ERR_NOMEM; }
    c->frames = f;
    f->d = *d;
    int st = ctx_alloc(c, &f->heads, (size_t)d->capacity * NHEAD, "frames heads");
    if (st == SPH_OK) st = ctx_alloc(c, &f->planes, (size_t)d->capacity * row, "frames log");
    if (st == SPH_OK) st = ctx_alloc(c, &f->w.ctl, 1, "frames words");
    if (st == SPH_OK) st = ctx_alloc(c, &f->w.part, (size_t)M_BLOCKS * NMX, "frames maxima");
    if (st == SPH_OK) st = ctx_alloc(c, &f->w.bad_part, (size_t)M_BLOCKS, "frames marks");
    if (st == SPH_OK) st = ctx_alloc(c, &f->w.limbs, limb_words(*d), "frames limbs");
    if (st != SPH_OK) { frames_free(c); return st; }
    frames_init<<<dim3(1), dim3(1), 0, c->stream>>>(f->w.ctl, c->d_dt);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { frames_free(c); SPH_HIP(e); }
    return SPH_OK;
}

int frames_end(sph_ctx *c) {
    if (!c->frames) { c->err = "sph_frames_end: no frames begun"; return SPH_ERR_STATE; }
    frames_free(c);
    return SPH_OK;
}

int frames_record(sph_ctx *c) {
    Frames *f = c->frames;
    if (!f) { c->err = "sph_frames_record: no frames begun"; return SPH_ERR_STATE; }
    return enqueue(c, f->d, f->w, f->heads, f->planes, f->d.capacity, true, (double)f->steps);
}

int frames_step(sph_ctx *c) {
    Frames *f = c->frames;
    if (!f) return SPH_OK;
    f->steps++;
    const bool by_step = f->d.every >= 1;
    if (by_step && f->steps % f->d.every != 0) return SPH_OK;
    return enqueue(c, f->d, f->w, f->heads, f->planes, f->d.capacity, by_step, (double)f->steps);
}

int frames_rewind(sph_ctx *c) {
    Frames *f = c->frames;
    if (!f) { c->err = "sph_frames_rewind: no frames begun"; return SPH_ERR_STATE; }
    SPH_HIP(hipMemsetAsync(&f->w.ctl->rows, 0, sizeof(long long), c->stream));
    return SPH_OK;
}

int frames_info(sph_ctx *c, int64_t *rows, int64_t *dropped, int64_t *steps) {
    const Frames *f = c->frames;
    if (!f) { c->err = "sph_frames_info: no frames begun"; return SPH_ERR_STATE; }
    if (steps) *steps = f->steps;
    if (rows || dropped) {                                 // the counts live on the device
        long long w[2] = {0, 0};
        SPH_HIP(hipMemcpyAsync(w, f->w.ctl, sizeof w, hipMemcpyDeviceToHost, c->stream));
        SPH_HIP(hipStreamSynchronize(c->stream));
        if (rows) *rows = w[0];
        if (dropped) *dropped = w[1];
    }
    return SPH_OK;
}

// the host cannot know the row count without waiting, so a range is checked against the capacity; rows that were never
// written hold what the allocation held
int frames_read(sph_ctx *c, int64_t first, int64_t count, double *head, double *planes, bool host) {
    const char *who = host ? "sph_frames_read" : "sph_frames_read_dev";
    const Frames *f = c->frames;
    if (!f) { c->err = std::string(who) + ": no frames begun"; return SPH_ERR_STATE; }
    int64_t limit = f->d.capacity;
    if (host) {
        int64_t rows = 0;
        SPH_TRY(frames_info(c, &rows, nullptr, nullptr));
        limit = rows;
    }
    if (first < 0 || count < 0 || first > limit || count > limit - first)
        return arg_error(c, who, host ? "first / count outside [0, rows]" : "first / count outside [0, capacity]");
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const size_t row = limb_words(f->d) / 2;
    if (count > 0 && head)
        SPH_HIP(hipMemcpyAsync(head, f->heads + (size_t)first * NHEAD, (size_t)count * NHEAD * sizeof(double), kind, c->stream));
    if (count > 0 && planes)
        SPH_HIP(hipMemcpyAsync(planes, f->planes + (size_t)first * row, (size_t)count * row * sizeof(double), kind, c->stream));
    return SPH_OK;
}

int frame_run(sph_ctx *c, const sph_frames_desc *d, double *head, double *planes, int64_t out_len, bool host) {
    const char *who = host ? "sph_frame" : "sph_frame_dev";
    SPH_TRY(check_desc(c, who, d, false));
    if (!head || !planes) return arg_error(c, who, "null output");
    const size_t row = limb_words(*d) / 2;
    if (out_len != (int64_t)row) return arg_error(c, who, "out_len does not match (1 + nq) n_u n_v");
    Work w{};
    double *d_head = nullptr, *d_planes = nullptr;
    auto layout = [&](Carve cv) {
        w.ctl = cv.take<Ctl>(1);
        w.part = cv.take<double>((size_t)M_BLOCKS * NMX);
        w.bad_part = cv.take<uint32_t>((size_t)M_BLOCKS);
        w.limbs = cv.take<unsigned long long>(limb_words(*d));
        d_head = cv.take<double>(host ? NHEAD : 0);
        d_planes = cv.take<double>(host ? row : 0);
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    frames_init<<<dim3(1), dim3(1), 0, c->stream>>>(w.ctl, c->d_dt);
    SPH_TRY(enqueue(c, *d, w, host ? d_head : head, host ? d_planes : planes, 1, true, c->frames ? (double)c->frames->steps : 0.0));
    if (host) {
        SPH_HIP(hipMemcpyAsync(head, d_head, NHEAD * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        SPH_HIP(hipMemcpyAsync(planes, d_planes, row * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    return SPH_OK;
}

}  // namespace sph
