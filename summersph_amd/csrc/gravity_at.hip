// gravity_at.hip -- the gravitational potential and acceleration at arbitrary points: the Barnes-Hut field of the gas
// sources and the field of the sinks (include/summersph.h, sph_gravity_at).
//
// Not part of the step loop: the state, the derived fields, the grid, the list, the statistics and dt stay as they are.
// As sph_energy, the tree of the sources is built into the context's tree arrays (gravity.hip, gravity_tree_build_records),
// which marks the context's own tree stale: the next sph_forces builds it again, bitwise the same.  The other scratch is
// the one the analysis calls share (analysis_scratch).
//
// Pipeline (all on ctx->stream):
//   [gas, no external sources]  stage_sources (energy.hip): {x, y, z, m} of the owned gas in the caller's order and their
//                               exact box, read back once (the tree's root box); the tree over the staged records
//   [gas, external sources]     the tree sph_forces builds over them, reused when it is in place
//   [gas]  gravat_point_keys    every point's 63-bit path key in the tree's root box (grav_keys' arithmetic on the point
//                               clamped into the box; a non-finite point sorts last), the point's index as value
//          rocprim radix sort   the walk order: 64 unrelated points share no part of their walks, 64 neighbours nearly all
//          grav_field_points    (gravity.hip) one wave per 64 points of the walk order: Phi and a of the gas, stored at the
//                               point's own index in rows 0-3 of the output
//   gravat_finish               one lane per point, in the caller's order: the sinks' Phi and a in sink order, the sum or the
//                               split rows, NaN rows for the points that cannot be evaluated, the two counts
// The point sort decides only which points share a wave; a lane's sums are its own walk's, so a point's rows depend on the
// sources, the sinks and the point alone.  No float atomics.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "sph_internal.hpp"

// the sink terms are written in one documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int PB = 256;                    // block of the per-point kernels
constexpr int KEY_LEVELS = 21;             // 3 bits per level: gravity.hip's path keys
constexpr double DBL_BIG = 1.7976931348623157e308;
constexpr uint64_t KEY_NONE = (uint64_t)1 << 63;      // a point without a place in the box: sorts last

struct Root { double c[3]; double size; };

__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return fabs(x) <= DBL_BIG && fabs(y) <= DBL_BIG && fabs(z) <= DBL_BIG;
}

__device__ __forceinline__ bool good_h(double h) { return h > 0.0 && h <= DBL_BIG; }

// the points' sort keys: the path of the point, clamped into the root box, down the octree of the sources ([F]:208-217)
__global__ __launch_bounds__(PB) void gravat_point_keys(Root rb, const double *__restrict__ px, const double *__restrict__ py,
                                                        const double *__restrict__ pz, int64_t m, uint64_t *__restrict__ keys,
                                                        uint32_t *__restrict__ vals) {
    const int64_t t = (int64_t)blockIdx.x * PB + threadIdx.x;
    if (t >= m) return;
    double x = px[t], y = py[t], z = pz[t];
    uint64_t key = KEY_NONE;
    if (finite3(x, y, z)) {
        const double half = 0.5 * rb.size;
        x = fmin(fmax(x, rb.c[0] - half), rb.c[0] + half);
        y = fmin(fmax(y, rb.c[1] - half), rb.c[1] + half);
        z = fmin(fmax(z, rb.c[2] - half), rb.c[2] + half);
        double cx = rb.c[0], cy = rb.c[1], cz = rb.c[2], size = rb.size;
        key = 0;
        for (int l = 0; l < KEY_LEVELS; l++) {
            const int bx = x > cx, by = y > cy, bz = z > cz;
            key = (key << 3) | (uint64_t)(bx | (by << 1) | (bz << 2));
            const double q = 0.25 * size;
            cx = cx + (bx ? q : -q); cy = cy + (by ? q : -q); cz = cz + (bz ? q : -q);
            size = size * 0.5;
        }
    }
    keys[t] = key;
    vals[t] = (uint32_t)t;
}

// One lane per point.  gas_walked: rows 0-3 of out hold the walk's result for the points it evaluated (0: the gas part is
// not asked for, or there is no source; it is 0.0 then).  The sinks' records come through the scalar cache (sink order,
// wave-uniform).
__global__ __launch_bounds__(PB) void gravat_finish(const double *__restrict__ px, const double *__restrict__ py,
                                                    const double *__restrict__ pz, const double *__restrict__ ph, double h_one,
                                                    int64_t m, const double *__restrict__ sink, int ns, double G, int flags,
                                                    int gas_walked, double *out, unsigned long long *__restrict__ counts) {
    const int64_t t = (int64_t)blockIdx.x * PB + threadIdx.x;
    const bool in = t < m;
    const int64_t i = in ? t : m - 1;
    const double x = px[i], y = py[i], z = pz[i];
    const double h = ph ? ph[i] : h_one;
    const bool fin = finite3(x, y, z), hok = good_h(h);
    const bool live = fin && hok;
    double g[4] = {0.0, 0.0, 0.0, 0.0}, s[4] = {0.0, 0.0, 0.0, 0.0};
    if (in && live && gas_walked)
        for (int c = 0; c < 4; c++) g[c] = out[c * m + i];
    if (in && live && (flags & SPH_GRAVAT_SINKS)) {
        for (int k = 0; k < ns; k++) {
            const double sm = sink[6 * MAX_SINKS + k];
            if (sm == 0.0) continue;
            const double dx = x - sink[k], dy = y - sink[MAX_SINKS + k], dz = z - sink[2 * MAX_SINKS + k];
            const double r = sqrt((dx * dx + dy * dy) + dz * dz);
            const double gm = G * sm;
            const double f = gm / ((r * r) * r);
            s[0] = s[0] - gm / r;
            s[1] = s[1] - f * dx; s[2] = s[2] - f * dy; s[3] = s[3] - f * dz;
        }
    }
    if (in) {
        const bool gas = (flags & SPH_GRAVAT_GAS) != 0, sinks = (flags & SPH_GRAVAT_SINKS) != 0;
        if (flags & SPH_GRAVAT_SPLIT) {
            for (int c = 0; c < 4; c++) {
                out[c * m + i] = live ? g[c] : NAN;
                out[(4 + c) * m + i] = live ? s[c] : NAN;
            }
        } else {
            for (int c = 0; c < 4; c++) out[c * m + i] = live ? (gas ? (sinks ? g[c] + s[c] : g[c]) : s[c]) : NAN;
        }
    }
    // counts: one integer atomic per wavefront and count
    const unsigned long long nonfin = __ballot(in && !fin);
    const unsigned long long badh = __ballot(in && !hok);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (nonfin) atomicAdd(&counts[0], (unsigned long long)__popcll(nonfin));
        if (badh) atomicAdd(&counts[1], (unsigned long long)__popcll(badh));
    }
}

}  // namespace

int gravity_at_run(sph_ctx *c, const sph_gravity_at_desc *d, int64_t n_points, const double *px, const double *py,
                   const double *pz, const double *ph, double *out, int64_t n_out, int64_t *counts, bool host) {
    const char *who = "sph_gravity_at";
    if (!d) return arg_error(c, who, "null descriptor");
    for (int k = 0; k < 3; k++)
        if (d->reserved[k] != 0) return arg_error(c, who, "reserved must be 0");
    const int flags = d->flags;
    if (flags & ~(SPH_GRAVAT_GAS | SPH_GRAVAT_SINKS | SPH_GRAVAT_SPLIT)) return arg_error(c, who, "unknown flags");
    const bool gas = (flags & SPH_GRAVAT_GAS) != 0, sinks = (flags & SPH_GRAVAT_SINKS) != 0, split = (flags & SPH_GRAVAT_SPLIT) != 0;
    if (!gas && !sinks) return arg_error(c, who, "no part selected (SPH_GRAVAT_GAS, SPH_GRAVAT_SINKS)");
    if (split && !(gas && sinks)) return arg_error(c, who, "SPH_GRAVAT_SPLIT needs both parts");
    if (n_points < 0 || n_points > 0x7fffffffLL) return arg_error(c, who, "n_points must be 0 .. 2^31 - 1");
    if (n_points > 0 && (!px || !py || !pz)) return arg_error(c, who, "null point arrays");
    if (n_out != (split ? 8 : 4) * n_points) return arg_error(c, who, "n_out != 4 n_points (8 n_points with SPH_GRAVAT_SPLIT)");
    if (!out && n_points > 0) return arg_error(c, who, "null output");
    if (std::isnan(d->h) || d->h < 0.0) return arg_error(c, who, "h must be >= 0");
    if (std::isnan(d->soft2) || d->soft2 < 0.0) return arg_error(c, who, "soft2 must be >= 0");
    if (!ph && !(d->h > 0.0) && c->variable) return arg_error(c, who, "h == 0 without ph on a variable-h context");
    const double h_one = ph ? 0.0 : (d->h > 0.0 ? d->h : c->p.h);
    if (!ph && !(h_one > 0.0)) {
        c->err = "sph_gravity_at: params.h <= 0 on a fixed-h context (give desc.h > 0 or ph)";
        return SPH_ERR_STATE;
    }
    hipStream_t st = c->stream;
    if (n_points == 0) {
        if (host) {
            if (counts) { counts[0] = 0; counts[1] = 0; }
        } else if (counts) {
            SPH_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
        }
        return SPH_OK;
    }

    const int64_t m = n_points;
    const bool ext = c->gx_src != nullptr;
    const int64_t no = c->n_owned;
    const int64_t n_src = gas ? (ext ? c->gx_n : no) : 0;
    const bool walk = n_src > 0;
    const bool stage = walk && !ext;
    const bool sort_points = walk && GravityAtSwitches().point_sort;      // A/B switch for the measurements of DESIGN.md section 14 (the results do not depend on it)
    const int nb = stage_blocks(no);
    size_t psort_bytes = 0;
    if (sort_points)
        SPH_HIP(rocprim::radix_sort_pairs(nullptr, psort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                          (uint32_t *)nullptr, (size_t)m, 0u, 64u, st));
    const size_t mp = sort_points ? (size_t)m : 0;
    double *rec, *box_part, *h_pts, *h_out;
    uint64_t *pkeys, *pkeys_alt;
    uint32_t *pvals, *pvals_alt;
    char *sort_tmp;
    unsigned long long *cnt;
    auto layout = [&](Carve cv) {
        rec = cv.take<double>(stage ? 4 * (size_t)no : 0);            // the staged records
        box_part = cv.take<double>(stage ? 6 * ((size_t)nb + 1) : 0);
        pkeys = cv.take<uint64_t>(mp);
        pkeys_alt = cv.take<uint64_t>(mp);
        pvals = cv.take<uint32_t>(mp);
        pvals_alt = cv.take<uint32_t>(mp);
        sort_tmp = cv.take<char>(psort_bytes);
        cnt = cv.take<unsigned long long>(2);
        h_pts = cv.take<double>(host ? (ph ? 4 : 3) * (size_t)m : 0);   // the host form's device copies
        h_out = cv.take<double>(host ? (size_t)n_out : 0);
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    SPH_TRY(analysis_pinned(c));
    const double *d_px = px, *d_py = py, *d_pz = pz, *d_ph = ph;
    if (host) {
        const double *src[4] = {px, py, pz, ph};
        for (int a = 0; a < (ph ? 4 : 3); a++)
            SPH_HIP(hipMemcpyAsync(h_pts + (size_t)a * m, src[a], (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        d_px = h_pts; d_py = h_pts + m; d_pz = h_pts + 2 * m;
        d_ph = ph ? h_pts + 3 * m : nullptr;
    }
    double *d_out = host ? h_out : out;
    SPH_HIP(hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned long long), st));

    if (walk) {
        Root rb;
        const double *bb = c->gx_box;
        double own[6];
        if (stage) {
            SPH_HIP(ensure_inv(c));
            SPH_TRY(stage_sources(c, rec, box_part, own));
            SPH_TRY(gravity_tree_build_records(c, rec, no, own));
            bb = own;
        } else if (!c->tree_valid) {
            // the tree sph_forces builds over the external sources (it does not depend on the context's own particles)
            double keep[4];
            for (int a = 0; a < 4; a++) keep[a] = c->root_box[a];
            SPH_TRY(gravity_tree_build(c));
            for (int a = 0; a < 4; a++) c->root_box[a] = keep[a];
            c->tree_rebuilt_for_analysis();
        }
        rb.size = 0.0;
        for (int a = 0; a < 3; a++) {                                  // the root box of the tree ([F]:803-808)
            rb.c[a] = (bb[3 + a] + bb[a]) / 2.0;
            rb.size = std::max(rb.size, bb[3 + a] - bb[a]);
        }
        if (sort_points) {
            gravat_point_keys<<<dim3(blocks(m, PB)), dim3(PB), 0, st>>>(rb, d_px, d_py, d_pz, m, pkeys, pvals);
            SPH_HIP(hipGetLastError());
            size_t tmp = psort_bytes;
            SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, pkeys, pkeys_alt, pvals, pvals_alt, (size_t)m, 0u, 64u, st));
        }
        SPH_HIP(launch_field_points(c, n_src, m, d_px, d_py, d_pz, d_ph, h_one, d->soft2, sort_points ? pvals_alt : nullptr, d_out));
    }
    gravat_finish<<<dim3(blocks(m, PB)), dim3(PB), 0, st>>>(d_px, d_py, d_pz, d_ph, h_one, m, c->sink, c->ns, c->p.G, flags,
                                                            walk ? 1 : 0, d_out, cnt);
    SPH_HIP(hipGetLastError());
    if (!host) {
        if (counts) SPH_HIP(hipMemcpyAsync(counts, cnt, 2 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        return SPH_OK;
    }
    SPH_HIP(hipMemcpyAsync(c->rnd_pinned, cnt, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipMemcpyAsync(out, d_out, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    int64_t cc[2] = {0, 0};
    std::memcpy(cc, c->rnd_pinned, sizeof(cc));
    if (counts) { counts[0] = cc[0]; counts[1] = cc[1]; }
    if (cc[1] > 0) {
        c->err = "sph_gravity_at: a point's softening length is <= 0 or non-finite";
        return SPH_ERR_STATE;
    }
    return SPH_OK;
}

}  // namespace sph
