// energy.hip -- conserved totals and the gravitational potential of a context (include/summersph.h, sph_energy).
//
// Not part of the step loop: the state, the derived fields, the grid, the list, the statistics and dt stay as they are.
// With SPH_FLAG_SELF_GRAVITY the Barnes-Hut tree of the potential is built into the context's tree arrays (gravity.hip,
// gravity_tree_build_records), which marks the context's own tree stale: the next sph_forces builds it again, bitwise the
// same.  The other scratch is the one the analysis calls share (analysis_scratch).
//
// Pipeline (all on ctx->stream):
//   [self-gravity, no external sources]
//     energy_stage     {x, y, z, m} of the owned gas in the caller's order (through inv) + per-block box partials
//     energy_box       the exact bounding box, read back once (the tree's root box)
//     tree over the staged records (gravity_tree_build_records)
//   [self-gravity, external sources: the tree sph_forces builds over them, reused when it is in place]
//   [self-gravity]      grav_potential_wave: Phi_self of every owned particle, by original id
//   energy_pieces      ids [1024 g, 1024 (g + 1)) of the caller's order by one wavefront (lane l: ids l, l + 64, ... in
//                      turn, then a xor butterfly over the 64 lanes): Phi_sink, phi = Phi_self + Phi_sink (optional output)
//                      and the 15 gas terms of each id, stored with plain stores at piece g
//   energy_final       one wavefront adds the pieces in the same shape; the sink terms (rank 0), the 28 sums
// The reduction shape depends only on the number of owned particles: the sums are bitwise independent of the context's
// sorted order, of the cell grid and of the launch.  No float atomics.
#include <cmath>
#include <vector>

#include "energy_terms.hpp"
#include "reduce_common.hpp"

// the per-particle arithmetic is written in one documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int NG = ENERGY_NG;          // gas sums (the terms: energy_terms.hpp)
constexpr int EB = 256;                // stage block
constexpr int BOX_BLOCKS = 1024;       // stage blocks at most (grid-stride beyond)

__global__ __launch_bounds__(EB) void energy_stage(const double *__restrict__ x, const double *__restrict__ y,
                                                   const double *__restrict__ z, const double *__restrict__ m,
                                                   const int32_t *__restrict__ inv, int64_t n, double4 *__restrict__ rec,
                                                   double *__restrict__ box_part) {
    __shared__ double lo[3][EB], hi[3][EB];
    double l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t k = (int64_t)blockIdx.x * EB + threadIdx.x; k < n; k += (int64_t)gridDim.x * EB) {
        const int32_t s = inv[k];
        const double4 r = make_double4(x[s], y[s], z[s], m[s]);
        rec[k] = r;
        l[0] = fmin(l[0], r.x); l[1] = fmin(l[1], r.y); l[2] = fmin(l[2], r.z);
        h[0] = fmax(h[0], r.x); h[1] = fmax(h[1], r.y); h[2] = fmax(h[2], r.z);
    }
    for (int a = 0; a < 3; a++) { lo[a][threadIdx.x] = l[a]; hi[a][threadIdx.x] = h[a]; }
    __syncthreads();
    for (int w = EB / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int a = 0; a < 3; a++) {
                lo[a][threadIdx.x] = fmin(lo[a][threadIdx.x], lo[a][threadIdx.x + w]);
                hi[a][threadIdx.x] = fmax(hi[a][threadIdx.x], hi[a][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 3) {
        box_part[blockIdx.x * 6 + threadIdx.x] = lo[threadIdx.x][0];
        box_part[blockIdx.x * 6 + 3 + threadIdx.x] = hi[threadIdx.x][0];
    }
}

// one wavefront: min / max over the blocks' partials -> out[0..6) (min xyz, max xyz)
__global__ __launch_bounds__(WAVE) void energy_box(const double *__restrict__ box_part, int nb, double *__restrict__ out) {
    const int lane = threadIdx.x;
    double v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int b = lane; b < nb; b += WAVE)
        for (int a = 0; a < 3; a++) {
            v[a] = fmin(v[a], box_part[b * 6 + a]);
            v[3 + a] = fmax(v[3 + a], box_part[b * 6 + 3 + a]);
        }
    for (int o = 32; o > 0; o >>= 1)
        for (int a = 0; a < 3; a++) {
            v[a] = fmin(v[a], __shfl_xor(v[a], o, 64));
            v[3 + a] = fmax(v[3 + a], __shfl_xor(v[3 + a], o, 64));
        }
    if (lane == 0)
        for (int a = 0; a < 6; a++) out[a] = v[a];
}

struct GasFields { const double *x, *y, *z, *vx, *vy, *vz, *u, *m; };

// one wavefront per piece of PIECE ids of the caller's order
__global__ __launch_bounds__(256) void energy_pieces(GasFields f, const int32_t *__restrict__ inv, int64_t n, int64_t n_pieces,
                                                     const double *__restrict__ sink, int ns, double G,
                                                     const double *__restrict__ phi_self, double *__restrict__ phi_out,
                                                     double *__restrict__ part) {
    const int64_t g = (int64_t)blockIdx.x * (256 / WAVE) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_pieces) return;
    const int64_t p1 = min(n, (g + 1) * PIECE);
    double acc[NG];
#pragma unroll
    for (int s = 0; s < NG; s++) acc[s] = 0.0;
    for (int64_t k = g * PIECE + lane; k < p1; k += WAVE) {
        const int32_t i = inv[k];
        const double x = f.x[i], y = f.y[i], z = f.z[i], vx = f.vx[i], vy = f.vy[i], vz = f.vz[i], m = f.m[i];
        const double ps = phi_sink(x, y, z, sink, ns, G);
        const double pg = phi_self ? phi_self[k] : 0.0;
        if (phi_out) phi_out[k] = pg + ps;
        double q[NG];
        gas_terms(x, y, z, vx, vy, vz, f.u[i], m, pg, ps, q);
#pragma unroll
        for (int s = 0; s < NG; s++) acc[s] += q[s];
    }
#pragma unroll
    for (int s = 0; s < NG; s++) acc[s] = wave_sum(acc[s]);
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NG; s++) part[g * NG + s] = acc[s];
    }
}

// one wavefront: the pieces (lane l: pieces l, l + 64, ... in turn, then the butterfly) -> sums[0..15); the sink part
// (rank 0; lane s: sink s, and its pair terms with the sinks t > s in t order) -> sums[15..28)
__global__ __launch_bounds__(WAVE) void energy_final(const double *__restrict__ part, int64_t n_pieces,
                                                     const double *__restrict__ sink, int ns, int rank0, double G,
                                                     double *__restrict__ sums) {
    const int lane = threadIdx.x;
    double acc[NG];
#pragma unroll
    for (int s = 0; s < NG; s++) acc[s] = 0.0;
    for (int64_t k = lane; k < n_pieces; k += WAVE) {
#pragma unroll
        for (int s = 0; s < NG; s++) acc[s] += part[k * NG + s];
    }
#pragma unroll
    for (int s = 0; s < NG; s++) acc[s] = wave_sum(acc[s]);
    constexpr int NK = ENERGY_NK;
    double sk[NK];
    sink_sums(lane, sink, ns, rank0, G, sk);
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < NG; s++) sums[s] = acc[s];
#pragma unroll
        for (int s = 0; s < NK; s++) sums[NG + s] = sk[s];
    }
}

}  // namespace

// The source set of sph_energy and sph_gravity_at without external sources: the owned gas as {x, y, z, m} records in the
// caller's order (rec: n_owned double4) and their exact box (bb: min xyz, max xyz; one read-back through the pinned slots,
// which the caller has made sure of).  box_part: 6 (stage_blocks + 1) doubles; c->inv is current (ensure_inv).
int stage_blocks(int64_t n_owned) {
    return (int)std::min<int64_t>((std::max<int64_t>(n_owned, 1) + EB - 1) / EB, BOX_BLOCKS);
}

int stage_sources(sph_ctx *c, double *rec, double *box_part, double bb[6]) {
    hipStream_t st = c->stream;
    const int64_t no = c->n_owned;
    const int nb = stage_blocks(no);
    double *box = box_part + 6 * (size_t)nb;
    energy_stage<<<dim3((unsigned)nb), dim3(EB), 0, st>>>(c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], c->f[SPH_F_M], c->inv, no,
                                                          reinterpret_cast<double4 *>(rec), box_part);
    energy_box<<<dim3(1), dim3(WAVE), 0, st>>>(box_part, nb, box);
    SPH_HIP(hipGetLastError());
    SPH_HIP(hipMemcpyAsync(c->rnd_pinned, box, 6 * sizeof(double), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    for (int a = 0; a < 6; a++) bb[a] = c->rnd_pinned[a];
    return SPH_OK;
}

int energy_sums(sph_ctx *c, int64_t src_offset, double *sums, double *phi, int64_t n_phi, bool host) {
    const char *who = "sph_energy";
    if (!sums && !phi) return arg_error(c, who, "both outputs are null");
    if (phi && n_phi != c->n) return arg_error(c, who, "n_phi != sph_count");
    const bool ext = c->gx_src != nullptr;
    const int64_t no = c->n_owned;
    if (ext && (src_offset < 0 || src_offset > c->gx_n - no))
        return arg_error(c, who, "src_offset out of range of the external sources");
    const bool self = c->gravity && no > 0;

    hipStream_t st = c->stream;
    const int64_t n_pieces = (no + PIECE - 1) / PIECE;
    const int64_t no1 = std::max<int64_t>(no, 1);
    const int nb = stage_blocks(no);
    double4 *rec;
    double *phi_buf, *box_part, *part, *sums_buf;
    auto layout = [&](Carve cv) {
        rec = cv.take<double4>(self && !ext ? no1 : 0);               // the staged records
        phi_buf = cv.take<double>(self ? no1 : 0);
        box_part = cv.take<double>(6 * ((size_t)nb + 1));             // the blocks' partials, then the box
        part = cv.take<double>(NG * (size_t)std::max<int64_t>(n_pieces, 1));
        sums_buf = cv.take<double>(SPH_ENERGY_NSUM);
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    double *phi_self = self ? phi_buf : nullptr;
    double *d_sums = host || !sums ? sums_buf : sums;
    double *d_phi = phi ? (host ? c->scratch : phi) : nullptr;      // host form: the download buffer (cap >= n doubles)
    SPH_TRY(analysis_pinned(c));
    SPH_HIP(ensure_inv(c));

    if (self) {
        int64_t n_src = no;
        if (!ext) {
            double bb[6];
            SPH_TRY(stage_sources(c, reinterpret_cast<double *>(rec), box_part, bb));
            SPH_TRY(gravity_tree_build_records(c, reinterpret_cast<const double *>(rec), no, bb));
            src_offset = 0;
        } else {
            // the tree sph_forces builds over the external sources (it does not depend on the context's own particles)
            n_src = c->gx_n;
            if (!c->tree_valid) {
                double rb[4];
                for (int a = 0; a < 4; a++) rb[a] = c->root_box[a];
                SPH_TRY(gravity_tree_build(c));
                for (int a = 0; a < 4; a++) c->root_box[a] = rb[a];
                c->tree_rebuilt_for_analysis();
            }
        }
        SPH_HIP(launch_potential(c, n_src, src_offset, phi_self));
    }
    if (n_pieces > 0) {
        GasFields gf{c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z], c->f[SPH_F_VX], c->f[SPH_F_VY], c->f[SPH_F_VZ], c->f[SPH_F_U],
                     c->f[SPH_F_M]};
        const int wpb = 256 / WAVE;
        energy_pieces<<<dim3((unsigned)((n_pieces + wpb - 1) / wpb)), dim3(256), 0, st>>>(gf, c->inv, no, n_pieces, c->sink, c->ns,
                                                                                         c->p.G, phi_self, d_phi, part);
    }
    if (d_phi && c->n > no) SPH_HIP(hipMemsetAsync(d_phi + no, 0, (size_t)(c->n - no) * sizeof(double), st));   // ghosts
    energy_final<<<dim3(1), dim3(WAVE), 0, st>>>(part, n_pieces, c->sink, c->ns, c->rank == 0 ? 1 : 0, c->p.G, d_sums);
    SPH_HIP(hipGetLastError());
    if (host) {
        if (sums) SPH_HIP(hipMemcpyAsync(sums, d_sums, SPH_ENERGY_NSUM * sizeof(double), hipMemcpyDeviceToHost, st));
        if (phi && c->n > 0) SPH_HIP(hipMemcpyAsync(phi, d_phi, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, st));
        SPH_HIP(hipStreamSynchronize(st));
    }
    return SPH_OK;
}

}  // namespace sph
