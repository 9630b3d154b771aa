// profile.hip -- azimuthally averaged disc profiles: mass-weighted moments of the owned gas particles binned into rings
// (and ring sectors) about a centre, in the frame of a disc normal (include/summersph.h, sph_profile).
//
// Not part of the step loop: nothing here reads or writes the context's grid, cell table, neighbour list, statistics or
// flags.  The scratch is the one the analysis calls share (analysis_scratch).
//
// Pipeline (all on ctx->stream):
//   [AUTO_NORMAL: the same four kernels over the spherical shell r_min <= |r'| < r_max as one bin, read-back of L]
//   profile_keys    every slot -> 64-bit key (bin << 32 | original id), slot; unselected slots get bin = n_bins, so
//                   the sort needs no count on the host and no compaction
//   rocprim radix sort on (bin, id)
//   profile_starts  start[b] = first sorted position of bin b (b in [0, n_bins]; start[n_bins] = selected count)
//   profile_pieces  bin b's run is cut into pieces of PIECE sorted positions from its own start; piece k of bin b is
//                   reduced by one wavefront (lane l adds positions l, l + 64, ... in turn, then a xor butterfly over the
//                   64 lanes) and stored with plain stores at slot start[b] / PIECE + b + k (injective in (b, k))
//   profile_final   one wavefront per bin adds its pieces (lane l: pieces l, l + 64, ... in turn, then the butterfly)
// Every bin's sums therefore have a reduction shape fixed by its start and length in the sorted (bin, id) sequence alone:
// bitwise independent of the context's slot order, of the cell grid and of the launch.  No float atomics.
#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <vector>

#include "disc_frame.hpp"
#include "reduce_common.hpp"

// the per-particle arithmetic is written in one documented order (summersph.h); no contraction into fused multiply-adds,
// so that a numpy restatement reproduces it
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int NS = SPH_PROFILE_NSUM;
constexpr int KB = 256;            // key / starts block

struct Bins {
    const double *edge;            // n_r + 1 ring edges
    double r_min, r_max, z_max;
    double guess_scale;            // linear: n_r / (r_max - r_min); log: n_r / log(r_max / r_min)
    int32_t n_r, n_phi, log, shell;   // shell: AUTO_NORMAL pass, r_min <= |r'| < r_max as bin 0
};

__global__ __launch_bounds__(KB) void profile_keys(const double *__restrict__ x, const double *__restrict__ y,
                                                   const double *__restrict__ z, const int32_t *__restrict__ orig,
                                                   int64_t n_slots, int64_t n_owned, DiscFrame f, Bins b, uint32_t n_bins,
                                                   uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * KB + threadIdx.x;
    if (i >= n_slots) return;
    const int32_t id = orig[i];
    uint32_t bin = n_bins;
    if (id < n_owned) {
        double c[3], cv[3], cm;
        centre_of(f, c, cv, cm);
        const Pos p = frame_pos(f, c, x[i], y[i], z[i]);
        if (b.shell) {
            const double r = sqrt((p.r[0] * p.r[0] + p.r[1] * p.r[1]) + p.r[2] * p.r[2]);
            if (r >= b.r_min && r < b.r_max) bin = 0;
        } else if (p.R >= b.r_min && p.R < b.r_max && fabs(p.Z) < b.z_max) {
            // a guess from the spacing, corrected against the host's edge table: edge[k] <= R < edge[k + 1]
            const double g = b.log ? log(p.R / b.r_min) * b.guess_scale : (p.R - b.r_min) * b.guess_scale;
            int k = (int)fmin(fmax(floor(g), 0.0), (double)(b.n_r - 1));
            while (k > 0 && p.R < b.edge[k]) k--;
            while (k < b.n_r - 1 && p.R >= b.edge[k + 1]) k++;
            int j = 0;
            if (b.n_phi > 1) {
                // sector j: -pi + 2 pi j / n_phi <= phi < -pi + 2 pi (j + 1) / n_phi, phi = atan2(Y, X) with +pi folded to -pi
                double phi = atan2(p.Y, p.X);
                if (phi >= M_PI) phi = -M_PI;
                const double twopi = 2.0 * M_PI;
                j = (int)fmin(fmax(floor((phi + M_PI) * ((double)b.n_phi / twopi)), 0.0), (double)(b.n_phi - 1));
                while (j > 0 && phi < -M_PI + (twopi * (double)j) / (double)b.n_phi) j--;
                while (j < b.n_phi - 1 && phi >= -M_PI + (twopi * (double)(j + 1)) / (double)b.n_phi) j++;
            }
            bin = (uint32_t)(k * b.n_phi + j);
        }
    }
    keys[i] = ((uint64_t)bin << 32) | (uint64_t)(uint32_t)id;
    vals[i] = (uint32_t)i;
}

// start[b] = lower bound of (b << 32) in the sorted keys, b in [0, n_bins]
__global__ __launch_bounds__(KB) void profile_starts(const uint64_t *__restrict__ keys, int64_t n, uint32_t n_bins,
                                                     int32_t *__restrict__ start) {
    const int64_t b = (int64_t)blockIdx.x * KB + threadIdx.x;
    if (b > (int64_t)n_bins) return;
    const uint64_t key = (uint64_t)b << 32;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    start[b] = (int32_t)lo;
}

// the 20 moments of one particle (summersph.h, "Raw sums"), added to acc in index order
__device__ __forceinline__ void add_moments(const DiscFrame &f, const double c[3], const double cv[3], double gm,
                                            const double *const *fld, int64_t i, double acc[NS]) {
    const Pos p = frame_pos(f, c, fld[0][i], fld[1][i], fld[2][i]);
    double v[3];
    v[0] = fld[3][i] - cv[0]; v[1] = fld[4][i] - cv[1]; v[2] = fld[5][i] - cv[2];
    const double v1 = dot3(v, f.e1), v2 = dot3(v, f.e2), vz = dot3(v, f.n);
    const double vR = p.R > 0.0 ? (p.X * v1 + p.Y * v2) / p.R : 0.0;
    const double vphi = p.R > 0.0 ? (p.X * v2 - p.Y * v1) / p.R : 0.0;
    const double l[3] = {p.r[1] * v[2] - p.r[2] * v[1], p.r[2] * v[0] - p.r[0] * v[2], p.r[0] * v[1] - p.r[1] * v[0]};
    double e[3] = {0.0, 0.0, 0.0};
    if (gm > 0.0) {
        const double r = sqrt((p.r[0] * p.r[0] + p.r[1] * p.r[1]) + p.r[2] * p.r[2]);
        const double w[3] = {v[1] * l[2] - v[2] * l[1], v[2] * l[0] - v[0] * l[2], v[0] * l[1] - v[1] * l[0]};
        for (int a = 0; a < 3; a++) e[a] = w[a] / gm - (r > 0.0 ? p.r[a] / r : 0.0);
    }
    const double m = fld[7][i];
    const double h = f.hf ? f.hf[i] : f.fixed_h;
    const double q[NS] = {1.0,           m,        m * p.R,        m * p.Z,        m * (p.Z * p.Z), m * vR, m * vphi,
                          m * vz,        m * (vR * vR), m * (vphi * vphi), m * (vz * vz), m * fld[6][i], m * fld[8][i],
                          m * h,         m * l[0], m * l[1],       m * l[2],       m * e[0],        m * e[1], m * e[2]};
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] += q[s];
}

struct Fields { const double *p[10]; };    // x y z vx vy vz u m alpha, [9] unused

// one wavefront per piece slot g; gaps (slots no (bin, piece) maps to) return at once
__global__ __launch_bounds__(KB) void profile_pieces(Fields fl, DiscFrame f, const uint32_t *__restrict__ vals, const int32_t *__restrict__ start,
                                                     uint32_t n_bins, int64_t n_pieces, double *__restrict__ part) {
    const int64_t g = (int64_t)blockIdx.x * (KB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_pieces) return;
    int64_t b, p0, p1;
    if (!piece_locate(start, (int64_t)n_bins, g, b, p0, p1)) return;
    double c[3], cv[3], cm;
    centre_of(f, c, cv, cm);
    const double gm = cm > 0.0 ? f.G * cm : 0.0;
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = 0.0;
    for (int64_t p = p0 + lane; p < p1; p += WAVE) add_moments(f, c, cv, gm, fl.p, (int64_t)vals[p], acc);
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = wave_sum(acc[s]);
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NS; s++) part[g * NS + s] = acc[s];
    }
}

// one wavefront per bin: its pieces in a fixed shape
__global__ __launch_bounds__(KB) void profile_final(const int32_t *__restrict__ start, uint32_t n_bins,
                                                    const double *__restrict__ part, double *__restrict__ sums) {
    const int64_t b = (int64_t)blockIdx.x * (KB / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= (int64_t)n_bins) return;
    const int64_t len = (int64_t)start[b + 1] - start[b];
    const int64_t np = (len + PIECE - 1) / PIECE, base = piece_base(start, b);
    double acc[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = 0.0;
    for (int64_t k = lane; k < np; k += WAVE) {
#pragma unroll
        for (int s = 0; s < NS; s++) acc[s] += part[(base + k) * NS + s];
    }
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = wave_sum(acc[s]);
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NS; s++) sums[b * NS + s] = acc[s];
    }
}

// the checks that need no context; what == null: fine
const char *check_desc(const sph_profile_desc *d, int64_t n_bins, bool need_normal) {
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return "reserved must be 0";
    if (d->flags & ~(SPH_PROFILE_LOG | SPH_PROFILE_AUTO_NORMAL)) return "unknown flags";
    if (d->n_r < 1 || d->n_phi < 1) return "n_r and n_phi must be >= 1";
    if ((int64_t)d->n_r * d->n_phi > ((int64_t)1 << 20)) return "n_r * n_phi must be <= 2^20";
    if (n_bins != (int64_t)d->n_r * d->n_phi) return "n_bins != n_r * n_phi";
    if (!std::isfinite(d->r_min) || !std::isfinite(d->r_max) || d->r_min < 0.0 || !(d->r_min < d->r_max))
        return "need finite 0 <= r_min < r_max";
    if ((d->flags & SPH_PROFILE_LOG) && d->r_min == 0.0) return "SPH_PROFILE_LOG needs r_min > 0";
    if (std::isnan(d->z_max)) return "z_max is NaN";
    if (need_normal) {
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(d->normal[a])) return "the normal is not finite";
        if (d->normal[0] == 0.0 && d->normal[1] == 0.0 && d->normal[2] == 0.0) return "the normal is zero";
    }
    return nullptr;
}

// edge[k], k in [0, n_r]: the frame header's table for the descriptor
void ring_edges(const sph_profile_desc *d, double *edge) {
    ring_edge_table(d->r_min, d->r_max, d->n_r, (d->flags & SPH_PROFILE_LOG) != 0, edge);
}

// the scratch of a pass (both passes of a call use the same)
struct PassBufs {
    uint64_t *keys, *keys_alt;
    uint32_t *vals, *vals_alt;
    char *sort_tmp;
    int32_t *start;
    double *part;
};

// one pass of the pipeline: the sums of n_bins bins into d_sums (device)
int run_pass(sph_ctx *c, const DiscFrame &f, const Bins &b, uint32_t n_bins, const PassBufs &pb, size_t sort_bytes, int64_t n_slots,
             double *d_sums) {
    hipStream_t st = c->stream;
    uint64_t *keys = pb.keys, *keys_alt = pb.keys_alt;
    uint32_t *vals = pb.vals, *vals_alt = pb.vals_alt;
    char *sort_tmp = pb.sort_tmp;
    int32_t *start = pb.start;
    double *part = pb.part;
    if (n_slots == 0) {
        SPH_HIP(hipMemsetAsync(d_sums, 0, (size_t)n_bins * NS * sizeof(double), st));
        return SPH_OK;
    }
    profile_keys<<<dim3((unsigned)((n_slots + KB - 1) / KB)), dim3(KB), 0, st>>>(
        c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], c->orig, n_slots, c->n_owned, f, b, n_bins, keys, vals);
    SPH_HIP(hipGetLastError());
    unsigned bbits = 1;
    while (bbits < 32 && ((uint64_t)1 << bbits) <= n_bins) bbits++;
    size_t tmp = sort_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, keys, keys_alt, vals, vals_alt, (size_t)n_slots, 0u, 32u + bbits, st));
    profile_starts<<<dim3((unsigned)((n_bins + 1 + KB - 1) / KB)), dim3(KB), 0, st>>>(keys_alt, n_slots, n_bins, start);
    const int64_t n_pieces = n_slots / PIECE + n_bins + 1;
    Fields fl{};
    for (int k = 0; k < 9; k++) fl.p[k] = c->f[k];
    const int wpb = KB / WAVE;
    profile_pieces<<<dim3((unsigned)((n_pieces + wpb - 1) / wpb)), dim3(KB), 0, st>>>(fl, f, vals_alt, start, n_bins,
                                                                                       n_pieces, part);
    profile_final<<<dim3((unsigned)((n_bins + wpb - 1) / wpb)), dim3(KB), 0, st>>>(start, n_bins, part, d_sums);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

}  // namespace

int profile_sums(sph_ctx *c, sph_profile_desc *d, double *sums, double *table, int64_t n_bins, bool host) {
    const char *who = "sph_profile";
    if (!d) return arg_error(c, who, "null descriptor");
    if (host ? (!sums && !table) : !sums) return arg_error(c, who, host ? "both outputs are null" : "null output");
    const bool autonorm = (d->flags & SPH_PROFILE_AUTO_NORMAL) != 0;
    if (const char *why = check_desc(d, n_bins, !autonorm)) return arg_error(c, who, why);
    if (d->sink < -1 || d->sink >= c->ns) return arg_error(c, who, "sink out of range");
    if (d->sink < 0)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(d->centre[a]) || !std::isfinite(d->centre_v[a])) return arg_error(c, who, "the centre is not finite");

    hipStream_t st = c->stream;
    const int64_t n_slots = c->cap > 0 ? c->n_slots : 0;
    const uint32_t nb = (uint32_t)n_bins;
    const int64_t n_pieces = n_slots / PIECE + n_bins + 1;
    size_t sort_bytes = 0;
    SPH_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)std::max<int64_t>(n_slots, 1), 0u, 64u, st));
    const int64_t ns1 = std::max<int64_t>(n_slots, 1);
    PassBufs pb{};
    double *d_edge, *h_sums, *d_auto;
    auto layout = [&](Carve cv) {
        pb.keys = cv.take<uint64_t>(ns1);
        pb.keys_alt = cv.take<uint64_t>(ns1);
        pb.vals = cv.take<uint32_t>(ns1);
        pb.vals_alt = cv.take<uint32_t>(ns1);
        pb.sort_tmp = cv.take<char>(sort_bytes);
        d_edge = cv.take<double>(d->n_r + 1);
        pb.start = cv.take<int32_t>(n_bins + 1);
        pb.part = cv.take<double>(NS * (size_t)n_pieces);
        h_sums = cv.take<double>(host ? NS * (size_t)n_bins : 0);     // the host form's device copy
        d_auto = cv.take<double>(NS);                                  // AUTO_NORMAL: the shell's sums
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    double *d_out = host ? h_sums : sums;
    SPH_TRY(analysis_pinned(c));

    DiscFrame f{};
    for (int a = 0; a < 3; a++) { f.c[a] = d->centre[a]; f.cv[a] = d->centre_v[a]; }
    f.cm = d->central_mass;
    f.G = c->p.G;
    f.fixed_h = c->p.h;
    f.hf = c->variable ? c->f[SPH_F_H] : nullptr;
    f.sink = c->sink;
    f.sink_k = d->sink;
    Bins b{};
    b.r_min = d->r_min; b.r_max = d->r_max; b.z_max = d->z_max;
    b.n_r = d->n_r; b.n_phi = d->n_phi; b.log = (d->flags & SPH_PROFILE_LOG) != 0;
    b.guess_scale = b.log ? (double)d->n_r / std::log(d->r_max / d->r_min) : (double)d->n_r / (d->r_max - d->r_min);
    b.edge = d_edge;

    double nrm[3];
    if (autonorm) {
        // the total angular momentum of the owned gas in the shell r_min <= |r'| < r_max, by the same sorted reduction
        const double ez[3] = {0.0, 0.0, 1.0};
        frame_axes(ez, f.n, f.e1, f.e2);
        Bins sb = b;
        sb.shell = 1;
        SPH_TRY(run_pass(c, f, sb, 1u, pb, sort_bytes, n_slots, d_auto));
        SPH_HIP(hipMemcpyAsync(c->rnd_pinned, d_auto + 14, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));
        for (int a = 0; a < 3; a++) nrm[a] = c->rnd_pinned[a];
        if (!(std::isfinite(nrm[0]) && std::isfinite(nrm[1]) && std::isfinite(nrm[2])) ||
            (nrm[0] == 0.0 && nrm[1] == 0.0 && nrm[2] == 0.0)) {
            c->err = "sph_profile: SPH_PROFILE_AUTO_NORMAL: the shell's angular momentum is zero or not finite";
            return SPH_ERR_STATE;
        }
    } else {
        for (int a = 0; a < 3; a++) nrm[a] = d->normal[a];
    }
    if (!frame_axes(nrm, f.n, f.e1, f.e2)) return arg_error(c, who, "the normal cannot be normalised");

    // the edge table travels in the stream's order from a pinned staging copy, rewritten only once its last upload is done
    const size_t ne = (size_t)d->n_r + 1;
    double *edge = nullptr;
    SPH_TRY(table_staging(c, ne, &edge));
    ring_edges(d, edge);
    for (int k = 0; k < d->n_r; k++)
        if (!(edge[k] < edge[k + 1])) return arg_error(c, who, "ring edges are not strictly increasing (rings too narrow)");
    SPH_HIP(hipMemcpyAsync(d_edge, edge, ne * sizeof(double), hipMemcpyHostToDevice, st));
    SPH_HIP(hipEventRecord(c->prf_evt, st));
    SPH_TRY(run_pass(c, f, b, nb, pb, sort_bytes, n_slots, d_out));
    if (host) {
        std::vector<double> hs;
        double *hsum = sums;
        if (!hsum) { hs.resize((size_t)n_bins * NS); hsum = hs.data(); }
        SPH_HIP(hipMemcpyAsync(hsum, d_out, (size_t)n_bins * NS * sizeof(double), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));
        for (int a = 0; a < 3; a++) d->normal[a] = f.n[a];
        if (table) return sph_profile_finish(d, &c->p, hsum, table, n_bins);
    } else {
        for (int a = 0; a < 3; a++) d->normal[a] = f.n[a];
    }
    return SPH_OK;
}

void profile_free(sph_ctx *c) {
    if (c->prf_evt) { (void)hipEventSynchronize(c->prf_evt); (void)hipEventDestroy(c->prf_evt); }
    if (c->prf_edge) (void)hipHostFree(c->prf_edge);
    c->prf_evt = nullptr; c->prf_edge = nullptr; c->prf_edge_cap = 0;
}

}  // namespace sph

extern "C" int sph_profile_finish(const sph_profile_desc *d, const sph_params *p, const double *sums, double *table,
                                  int64_t n_bins) {
    using namespace sph;
    if (!d || !p || !sums || !table) return SPH_ERR_ARG;
    if (check_desc(d, n_bins, true)) return SPH_ERR_ARG;
    double n[3], e1[3], e2[3];
    if (!frame_axes(d->normal, n, e1, e2)) return SPH_ERR_ARG;
    const int nr = d->n_r, nphi = d->n_phi;
    std::vector<double> edge((size_t)nr + 1);
    ring_edges(d, edge.data());
    const double nan = NAN, pi = M_PI, twopi = 2.0 * M_PI;

    // ring-combined <R> and Omega (sectors added in j order), f = R^4 Omega^2
    std::vector<double> rr(nr), ff(nr), k2(nr);
    for (int k = 0; k < nr; k++) {
        double m = 0.0, mr = 0.0, mvp = 0.0;
        for (int j = 0; j < nphi; j++) {
            const double *s = sums + ((int64_t)k * nphi + j) * NS;
            m += s[1]; mr += s[2]; mvp += s[6];
        }
        const double R = mr / m, om = (mvp / m) / R;
        rr[k] = R;
        ff[k] = ((R * R) * (R * R)) * (om * om);
    }
    for (int k = 0; k < nr; k++) {
        double df = nan;
        if (nr > 1) {
            const int a = k == 0 ? 0 : k - 1, b = k == nr - 1 ? nr - 1 : k + 1;
            df = (ff[b] - ff[a]) / (rr[b] - rr[a]);
        }
        k2[k] = df / ((rr[k] * rr[k]) * rr[k]);
    }

    for (int k = 0; k < nr; k++) {
        for (int j = 0; j < nphi; j++) {
            const int64_t bi = (int64_t)k * nphi + j;
            const double *s = sums + bi * NS;
            double *t = table + bi * SPH_PROFILE_NCOL;
            const double M = s[1];
            const double area = (pi * (edge[k + 1] * edge[k + 1] - edge[k] * edge[k])) / (double)nphi;
            const double sig = M / area;
            auto mean = [&](int q) { return s[q] / M; };
            auto disp = [&](int q1, int q2) {
                const double mu = mean(q1), var = mean(q2) - mu * mu;
                return var < 0.0 ? 0.0 : std::sqrt(var);
            };
            t[0] = edge[k];
            t[1] = edge[k + 1];
            t[2] = mean(2);
            t[3] = s[0];
            t[4] = M;
            t[5] = sig;
            t[6] = mean(3);
            t[7] = disp(3, 4);
            t[8] = mean(5);
            t[9] = mean(6);
            t[10] = mean(7);
            t[11] = disp(5, 8);
            t[12] = disp(6, 9);
            t[13] = disp(7, 10);
            t[14] = mean(11);
            const double cs2 = (p->gamma * p->gamma_m1) * t[14];
            t[15] = cs2 < 0.0 ? nan : std::sqrt(cs2);
            t[16] = mean(12);
            t[17] = mean(13);
            t[18] = t[9] / t[2];
            const double kappa = k2[k] < 0.0 ? nan : std::sqrt(k2[k]);
            t[19] = kappa;
            t[20] = sig == 0.0 ? nan : (t[15] * kappa) / ((pi * p->G) * sig);
            t[21] = -(((twopi * t[2]) * sig) * t[8]);
            const double L[3] = {s[14], s[15], s[16]};
            const double Ln = std::sqrt((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]);
            t[22] = Ln / M;
            double lh[3];
            for (int a = 0; a < 3; a++) lh[a] = L[a] / Ln;
            // tilt = atan2(|L^ x n^|, L^.n^) with |L^ x n^| = sqrt(a1^2 + a2^2): acos(L^.n^) loses accuracy near 0
            const double a1 = (lh[0] * e1[0] + lh[1] * e1[1]) + lh[2] * e1[2], a2 = (lh[0] * e2[0] + lh[1] * e2[1]) + lh[2] * e2[2];
            const double a3 = (lh[0] * n[0] + lh[1] * n[1]) + lh[2] * n[2];
            t[23] = std::atan2(std::sqrt(a1 * a1 + a2 * a2), a3);
            t[24] = std::atan2(a2, a1);
            const double E[3] = {s[17], s[18], s[19]};
            t[25] = std::sqrt((E[0] * E[0] + E[1] * E[1]) + E[2] * E[2]) / M;
            t[26] = M == 0.0 ? nan
                             : std::atan2((E[0] * e2[0] + E[1] * e2[1]) + E[2] * e2[2], (E[0] * e1[0] + E[1] * e1[1]) + E[2] * e1[2]);
            t[27] = -pi + (twopi * (double)j) / (double)nphi;
            t[28] = -pi + (twopi * (double)(j + 1)) / (double)nphi;
        }
    }
    return SPH_OK;
}
