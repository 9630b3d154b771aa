// terms.hip -- the rates of sph_forces split by physical term (include/summersph.h, sph_force_terms): pressure gradient,
// artificial viscosity, sink gravity, gas self-gravity, PdV work, viscous heating and the two addends of the alpha rate,
// per owned particle, from the context's own neighbour lists and force records.
//
// Not part of the step loop: it reads the lists and records the step made and writes nothing the step reads.
//
//   fixed h     force_terms_kernel<BLOCK, PACKED>   the gather form of forces_kernel (pairs.hip): one lane per target, the dw
//                                                   table in LDS, ListColumn<PACKED> (both list layouts), the neighbour record
//                                                   fetched a trip ahead and its index two, wave_max trips, XCD chunking
//   variable h  force_terms_v_kernel                the same of forces_v_kernel (varh.hip): whole list rows streamed two ahead,
//                                                   the entries' F flag honoured (density-only entries add nothing)
//   gravity     launch_gravity (gravity.hip)        the walk of sph_forces, writing to this call's scratch instead of
//                                                   SPH_F_AX..AZ
// The visits (force_visit_terms, force_visit_terms_v) are force_visit's and force_visit_v's arithmetic with the one
// accumulator mC = m_j ((P_i/rho_i^2 + P_j/rho_j^2) + visc) taken apart: nine running sums instead of five.  The epilogues
// compute the sink loop from zero, apply the normalisation once and store the particle's sixteen values as one 128-byte
// record at its slot (the lanes of ghosts store NaN); terms_rows turns the records into rows at the original ids.
#include <cmath>

#include "pair_common.hpp"
#include "tile_common.hpp"

namespace sph {

namespace {

constexpr int TBLOCK = 256;

// un-normalised sums of one target: a_P (3), a_V (3), du_P, du_V and the alpha source's sum m_j v_ij . grad W
struct TermSums { double p0 = 0.0, p1 = 0.0, p2 = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0, duP = 0.0, duV = 0.0, sdal = 0.0; };

// one visit of the fixed-h sums, [F]:356-391 -- force_visit (pair_common.hpp) line by line up to visc; then the pressure part
// (C.z + j.P_r2) and the viscous part visc of [F]:381-382 go to sums of their own, and so do the two parts of [F]:387.  No
// control flow: beyond 2h and at r == 0 the knots give g = 0, and every term is an exact zero.
template <class DwFn>
__device__ __forceinline__ void force_visit_terms(const PairConst &pc, double inv_h, const double4 &A, const double4 &B,
                                                  const double4 &C, const Nbr &j, bool act, DwFn dw_of, TermSums &f) {
#pragma clang fp contract(off)
    const double n0 = A.x - j.x, n1 = A.y - j.y, n2 = A.z - j.z;                  // [F]:356
    const double r2 = fma(n2, n2, fma(n1, n1, n0 * n0));
    double dr, rs;
    rsqrt_sqrt(r2, dr, rs);                                                       // [F]:357
    const double qi = dr * inv_h;
    const Knots kn = dw_of(qi);
    const double v0 = B.x - j.vx, v1 = B.y - j.vy, v2 = B.z - j.vz;               // [F]:358
    const double vdotr = fmin(fma(v2, n2, fma(v1, n1, v0 * n0)), 0.0);            // [F]:359-361
    double inv_r2e, inv_rho;
    rcp_pair(r2 + pc.visc_eps_h2, B.w + j.rho_h, inv_r2e, inv_rho);
    const double vis_nu = (pc.h * vdotr) * inv_r2e;                               // [F]:373
    const double cbar = C.x + j.c_h;                                              // [F]:374 (halves stored)
    const double abar = C.y + j.al_h;                                             // [F]:376
    const double visc = ((abar * vis_nu) * fma(2.0, vis_nu, -cbar)) * inv_rho;    // [F]:378: Pi_ij
    const double mj = act ? j.m : 0.0;
    const double mP = mj * (C.z + j.P_r2);                                        // [F]:381-382, the pressure part
    const double mV = mj * visc;                                                  //              the viscous part
    const double dWm = knots_value(kn) * rs;                                      // [F]:366
    const double g0 = n0 * dWm, g1 = n1 * dWm, g2 = n2 * dWm;                     // [F]:363,368
    const double vdotgradW = fma(g2, v2, fma(g1, v1, g0 * v0));                   // [F]:370
    f.p0 = fma(mP, g0, f.p0); f.p1 = fma(mP, g1, f.p1); f.p2 = fma(mP, g2, f.p2); // [F]:383
    f.v0 = fma(mV, g0, f.v0); f.v1 = fma(mV, g1, f.v1); f.v2 = fma(mV, g2, f.v2);
    const double mv = mj * vdotgradW;
    f.duP = fma(mv, C.z, f.duP);                                                  // [F]:387, P_i/rho_i^2
    f.duV = fma(mv, 0.5 * visc, f.duV);                                           //          visc/2
    f.sdal = f.sdal + mv;                                                         // [F]:390
}

// one visit of the grad-h sums, [V]:385-427 -- force_visit_v (varh.hip) with S = (C_i dW_i + C_j dW_j + visc dW_s) / r taken
// apart into its first two addends and its third ([V]:413-414), and [V]:419-421 into C_i and visc/2
__device__ __forceinline__ void force_visit_terms_v(const PairConst &pc, double hi, double inv_h, double inv_dq, double inv_pi,
                                                    double inv_n4i, const double *__restrict__ lds_dw, const double4 &A,
                                                    const double4 &B, const double4 &Cc, const double4 &Aj, const double4 &Bj,
                                                    const double4 &Cj, bool act, TermSums &f) {
    const double n0 = A.x - Aj.x, n1 = A.y - Aj.y, n2 = A.z - Aj.z;                   // [V]:385
    const double r2 = n0 * n0 + n1 * n1 + n2 * n2;
    double dr, rs;
    rsqrt_sqrt(r2, dr, rs);
    if (act && r2 > 0.0) {
        const double hj = Cj.w;
        const double inv_hj = fast_rcp(hj);
        const double qo = dr * inv_h, qn = dr * inv_hj;
        const double ihj2 = inv_hj * inv_hj;
        const double dWo = qo <= 2.0 ? table_lerp(lds_dw, qo, inv_dq, pc.nq) * inv_n4i : 0.0;       // [V]:395-396,140
        const double dWn = qn <= 2.0 ? table_lerp(lds_dw, qn, inv_dq, pc.nq) * (ihj2 * ihj2 * inv_pi) : 0.0;
        const double v0 = B.x - Bj.x, v1 = B.y - Bj.y, v2 = B.z - Bj.z;               // [V]:387
        const double vr = v0 * n0 + v1 * n1 + v2 * n2;
        const double vdotr = fmin(vr, 0.0);                                           // [V]:388-390
        const double dWs = 0.5 * (dWo + dWn);
        const double vdotgradW = (vr * rs) * dWs;                                     // [V]:401
        const double avg_len = 0.5 * (hi + hj);                                       // [V]:402
        double inv_r2e, inv_rho;
        rcp_pair(r2 + pc.visc_eps_h2 * avg_len * avg_len, B.w + Bj.w, inv_r2e, inv_rho);
        const double vis_nu = (avg_len * vdotr) * inv_r2e;                            // [V]:405
        const double cbar = Cc.x + Cj.x, abar = Cc.y + Cj.y;
        const double visc = (abar * vis_nu) * (2.0 * vis_nu - cbar) * inv_rho;        // [V]:410: Pi_ij
        const double mSP = Aj.w * ((Cc.z * dWo + Cj.z * dWn) * rs);                   // [V]:413-414, C_i g_i + C_j g_j (along n)
        const double mSV = Aj.w * ((visc * dWs) * rs);                                //              Pi_ij (g_i + g_j) / 2
        f.p0 = fma(mSP, n0, f.p0); f.p1 = fma(mSP, n1, f.p1); f.p2 = fma(mSP, n2, f.p2);   // [V]:416
        f.v0 = fma(mSV, n0, f.v0); f.v1 = fma(mSV, n1, f.v1); f.v2 = fma(mSV, n2, f.v2);
        const double mv = Aj.w * vdotgradW;
        f.duP = fma(mv, Cc.z, f.duP);                                                 // [V]:419-421, C_i
        f.duV = fma(mv, 0.5 * visc, f.duV);                                           //              visc/2
        f.sdal += mv;                                                                 // [V]:427
    }
}

// The sixteen values of a particle go to one 128-byte record at its slot: a full cache line per lane, a wave writes 8 KB in a
// row.  (Stored straight to the rows, out[row * n + original id], they are sixteen 8-byte stores per lane, each to a line of
// its own, because the original ids of a wave's lanes are scattered: 0.72 instead of 0.49 ms per call on the 10^6 disc,
// DESIGN.md section 17.)  terms_rows then turns the records into rows.
__device__ __forceinline__ void store_values(double *__restrict__ rec, int64_t slot, const double (&v)[SPH_TERMS_NROW]) {
    double4 *o = reinterpret_cast<double4 *>(rec + (size_t)slot * SPH_TERMS_NROW);
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = make_double4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
}
__device__ __forceinline__ void store_nan_values(double *__restrict__ rec, int64_t slot) {
    double v[SPH_TERMS_NROW];
#pragma unroll
    for (int k = 0; k < SPH_TERMS_NROW; k++) v[k] = NAN;
    store_values(rec, slot, v);
}

// records in slot order -> rows in the caller's order: lane = original id, its record is one cache line
__global__ __launch_bounds__(256) void terms_rows(const double *__restrict__ rec, const int32_t *__restrict__ inv, int64_t n,
                                                  double *__restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const double4 *r = reinterpret_cast<const double4 *>(rec + (size_t)inv[id] * SPH_TERMS_NROW);
    const double4 a = r[0], b = r[1], c = r[2], d = r[3];
    double *o = out + id;
    o[0] = a.x; o[(size_t)n] = a.y; o[(size_t)2 * n] = a.z; o[(size_t)3 * n] = a.w;
    o[(size_t)4 * n] = b.x; o[(size_t)5 * n] = b.y; o[(size_t)6 * n] = b.z; o[(size_t)7 * n] = b.w;
    o[(size_t)8 * n] = c.x; o[(size_t)9 * n] = c.y; o[(size_t)10 * n] = c.z; o[(size_t)11 * n] = c.w;
    o[(size_t)12 * n] = d.x; o[(size_t)13 * n] = d.y; o[(size_t)14 * n] = d.z; o[(size_t)15 * n] = d.w;
}

// rows 9-11: grav_mode 0 -> +0.0 (no self-gravity), 1 -> NaN (SPH_TERMS_SKIP_GAS_GRAVITY), 2 -> the walk's term at slot i
__device__ __forceinline__ void gravity_rows(int grav_mode, const double *__restrict__ g, int64_t n, int64_t i, double *a) {
#pragma unroll
    for (int k = 0; k < 3; k++) a[k] = grav_mode == 2 ? g[(size_t)k * n + i] : (grav_mode == 1 ? NAN : 0.0);
}

template <int BLOCK, bool PACKED>
__global__ __launch_bounds__(BLOCK) void force_terms_kernel(PairConst pc, const double *__restrict__ frec,
                                                            const int32_t *__restrict__ nlist, int32_t cap,
                                                            const int32_t *__restrict__ ncount,
                                                            const int32_t *__restrict__ wave_max,
                                                            const double *__restrict__ dw_tab, const double *__restrict__ sink,
                                                            int64_t n, const int32_t *__restrict__ orig, int32_t n_owned,
                                                            const int32_t *__restrict__ plan_f, int grav_mode,
                                                            const double *__restrict__ grav, double *__restrict__ rec) {
    extern __shared__ double lds_dw[];
    for (int k = threadIdx.x; k < TAB_LEN(pc.nq); k += BLOCK) lds_dw[k] = dw_tab[k];
    __syncthreads();

    const int64_t i = (int64_t)xcd_chunk(blockIdx.x, gridDim.x) * BLOCK + threadIdx.x;
    if ((i & ~(int64_t)63) >= n) return;
    const int lane = threadIdx.x & 63;
    const int64_t w = i >> 6;
    const bool live = i < n && orig[i] < n_owned;
    const int self = i < n ? (int)i : (int)(n - 1);
    const double4 *fi = reinterpret_cast<const double4 *>(frec + (size_t)self * FREC);
    const double4 A = fi[0], B = fi[1], Cc = fi[2];   // x y z m | vx vy vz rho/2 | c/2 alpha/2 P/rho^2 -
    const int cnt = live ? min(ncount[i], cap) : 0;
    const int kmax = wave_max[w];
    const ListColumn<PACKED> mine(nlist, plan_f, w, cap, lane, self);
    const double inv_h = pc.inv_h, inv_dq = pc.inv_dq;

    TermSums f;
    auto dw_of = [&](double q) { return table_knots_at(lds_dw, knot_coord(q, inv_dq)); };
    int j1 = 0 < cnt ? mine(0) : self;
    int j2 = 1 < cnt ? mine(1) : self;
    const double4 *fj = reinterpret_cast<const double4 *>(frec + (size_t)j1 * FREC);
    double4 A1 = fj[0], B1 = fj[1], C1 = fj[2];
    for (int k = 0; k < kmax; k++) {
        const Nbr nb = nbr_of(A1, B1, C1);
        const bool act = k < cnt;
        j1 = j2;
        if (k + 2 < cnt) j2 = mine(k + 2);
        if (k + 1 < cnt) {                       // idle lanes issue no gather
            fj = reinterpret_cast<const double4 *>(frec + (size_t)j1 * FREC);
            A1 = fj[0]; B1 = fj[1]; C1 = fj[2];
        }
        force_visit_terms(pc, inv_h, A, B, Cc, nb, act, dw_of, f);
    }
    if (i >= n) return;
    if (!live) { store_nan_values(rec, i); return; }      // a ghost: a source only

    // force_epilogue (pair_common.hpp) term by term: a_P | a_V | a_S | a_G | du_P du_V | alpha source, decay
    {
#pragma clang fp contract(off)
        double v[SPH_TERMS_NROW];
        const SinkRows sk = sink_rows(sink);
        const ForceSums none;                                   // the sink loop of force_channel alone, started from 0
        v[0] = 0.0 - f.p0 * pc.inv_dwnorm; v[1] = 0.0 - f.p1 * pc.inv_dwnorm; v[2] = 0.0 - f.p2 * pc.inv_dwnorm;   // [F]:383, [F]:126 once
        v[3] = 0.0 - f.v0 * pc.inv_dwnorm; v[4] = 0.0 - f.v1 * pc.inv_dwnorm; v[5] = 0.0 - f.v2 * pc.inv_dwnorm;
        v[6] = force_channel(pc, sk, A, none, 0.0, 0);
        v[7] = force_channel(pc, sk, A, none, 0.0, 1);
        v[8] = force_channel(pc, sk, A, none, 0.0, 2);
        gravity_rows(grav_mode, grav, n, i, v + 9);
        v[12] = f.duP * pc.inv_dwnorm; v[13] = f.duV * pc.inv_dwnorm;                                              // [F]:387
        v[14] = fmax((f.sdal * pc.inv_dwnorm) * fast_rcp(2.0 * B.w), 0.0);                                         // [F]:316-318,390
        v[15] = pc.alpha_decay * (((pc.alpha_floor - 2.0 * Cc.y) * (2.0 * Cc.x)) * inv_h);
        store_values(rec, i, v);
    }
}

__global__ __launch_bounds__(TBLOCK) void force_terms_v_kernel(PairConst pc, const double *__restrict__ frec,
                                                               const int32_t *__restrict__ nlist, int32_t cap,
                                                               const int32_t *__restrict__ ncount,
                                                               const int32_t *__restrict__ wave_max,
                                                               const double *__restrict__ dw_tab, const double *__restrict__ sink,
                                                               int64_t n, const int32_t *__restrict__ orig, int32_t n_owned,
                                                               int grav_mode, const double *__restrict__ grav,
                                                               double *__restrict__ rec) {
    extern __shared__ double lds_dw[];
    for (int k = threadIdx.x; k < TAB_LEN(pc.nq); k += TBLOCK) lds_dw[k] = dw_tab[k];
    __syncthreads();

    const int64_t i = (int64_t)xcd_chunk(blockIdx.x, gridDim.x) * TBLOCK + threadIdx.x;
    if ((i & ~(int64_t)63) >= n) return;
    const int lane = threadIdx.x & 63;
    const int64_t w = i >> 6;
    const bool live = i < n && orig[i] < n_owned;
    const int self = i < n ? (int)i : (int)(n - 1);
    const double4 *fi = reinterpret_cast<const double4 *>(frec + (size_t)self * FREC);
    const double4 A = fi[0], B = fi[1], Cc = fi[2];   // x y z m | vx vy vz rho/2 | c/2 alpha/2 P/(Om rho^2) h
    const int cnt = live ? min(ncount[i], cap) : 0;
    const int kmax = __builtin_amdgcn_readfirstlane(wave_max[w]);
    const int4 *mine4 = reinterpret_cast<const int4 *>(nlist) + ((size_t)w * (cap >> 2)) * 64 + lane;
    const double hi = Cc.w;
    const double inv_h = 1.0 / hi, inv_dq = 0.5 * pc.nq, inv_pi = 1.0 / pc.kernel_pi;
    const double inv_n4i = 1.0 / (pc.kernel_pi * ((hi * hi) * (hi * hi)));          // [V]:140 for h_i

    TermSums f;
    const int nrow = (kmax + 3) >> 2;
    int4 qa = make_int4(0, 0, 0, 0), qb = qa;
    if (kmax > 0) { qa = load_row(mine4); qb = load_row(mine4 + (size_t)min(1, nrow - 1) * 64); }
    int e1 = 0 < cnt ? qa.x : self;
    const double4 *fj = reinterpret_cast<const double4 *>(frec + (size_t)(e1 & IDX_MASK) * FREC);
    double4 A1 = fj[0], B1 = fj[1], C1 = fj[2];
    for (int r = 0; r < nrow; r++) {                  // whole rows (four entries), rows streamed two ahead
        const int4 qc = load_row(mine4 + (size_t)min(r + 2, nrow - 1) * 64);
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int k = 4 * r + v;
            const double4 Aj = A1, Bj = B1, Cj = C1;
            const bool act = k < cnt && ((uint32_t)e1 & FLAG_F);       // density-only entries, one-sided pairs: no F, no term
            if (k + 1 < cnt) {                          // idle lanes issue no gather
                e1 = v < 3 ? comp4(qa, v + 1) : qb.x;
                fj = reinterpret_cast<const double4 *>(frec + (size_t)(e1 & IDX_MASK) * FREC);
                A1 = fj[0]; B1 = fj[1]; C1 = fj[2];
            }
            force_visit_terms_v(pc, hi, inv_h, inv_dq, inv_pi, inv_n4i, lds_dw, A, B, Cc, Aj, Bj, Cj, act, f);
        }
        qa = qb; qb = qc;
    }
    if (i >= n) return;
    if (!live) { store_nan_values(rec, i); return; }

    // force_epilogue_v (varh.hip) term by term
    double v[SPH_TERMS_NROW];
    PairConst sinks_only = pc;
    sinks_only.grav = 0;                                // sink_gas_accel's loop, started from 0
    sink_gas_accel(sinks_only, sink, A, i, nullptr, nullptr, nullptr, v[6], v[7], v[8]);
    v[0] = 0.0 - f.p0; v[1] = 0.0 - f.p1; v[2] = 0.0 - f.p2;
    v[3] = 0.0 - f.v0; v[4] = 0.0 - f.v1; v[5] = 0.0 - f.v2;
    gravity_rows(grav_mode, grav, n, i, v + 9);
    v[12] = f.duP; v[13] = f.duV;
    v[14] = fmax(f.sdal / (2.0 * B.w), 0.0);                                                            // [V]:346
    v[15] = pc.alpha_decay * ((pc.alpha_floor - 2.0 * Cc.y) * (2.0 * Cc.x) / hi);
    store_values(rec, i, v);
}

}  // namespace

int force_terms_run(sph_ctx *c, const sph_force_terms_desc *d, double *out, int64_t n_out, bool host) {
    const char *who = "sph_force_terms";
    if (!d) return arg_error(c, who, "null descriptor");
    for (int k = 0; k < 3; k++)
        if (d->reserved[k] != 0) return arg_error(c, who, "reserved must be 0");
    if (d->flags & ~SPH_TERMS_SKIP_GAS_GRAVITY) return arg_error(c, who, "unknown flags");
    const int64_t n = c->n;
    if (n_out != (int64_t)SPH_TERMS_NROW * n) return arg_error(c, who, "n_out != SPH_TERMS_NROW * sph_count");
    if (!out && n > 0) return arg_error(c, who, "null output");
    if (n == 0) return SPH_OK;
    if (!c->eos_valid || !c->grid_valid) { c->err = "sph_force_terms: call sph_density first"; return SPH_ERR_STATE; }

    hipStream_t st = c->stream;
    const bool skip = (d->flags & SPH_TERMS_SKIP_GAS_GRAVITY) != 0;
    const bool walk = c->gravity && !skip;
    const int grav_mode = walk ? 2 : (skip ? 1 : 0);
    double *grav, *rec, *h_out;
    auto layout = [&](Carve cv) {
        grav = cv.take<double>(walk ? 3 * (size_t)n : 0);              // the walk's term, slot order
        rec = cv.take<double>((size_t)n_out);                          // the sixteen values of every slot
        h_out = cv.take<double>(host ? (size_t)n_out : 0);             // the host form's device copy
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    double *d_out = host ? h_out : out;

    if (walk) {
        // the tree sph_forces would build (and keeps): built here when none is in place, and kept for it
        if (!c->tree_valid) { SPH_TRY(gravity_tree_build(c)); c->tree_valid = true; }
        SPH_HIP(hipMemsetAsync(grav, 0, 3 * (size_t)n * sizeof(double), st));      // an empty external source set: no walk, zeros
        SPH_HIP(launch_gravity(c, grav, grav + n, grav + 2 * n));
    }
    PairConst pc = make_pair_const(c);
    const size_t lds = (size_t)TAB_LEN(pc.nq) * sizeof(double);
    const dim3 grid((unsigned)((n + TBLOCK - 1) / TBLOCK)), block(TBLOCK);
    if (c->variable) {
        force_terms_v_kernel<<<grid, block, lds, st>>>(pc, c->frec, c->nlist, c->nl_cap, c->ncount, c->wave_max, c->dw_tab, c->sink,
                                                       n, c->orig, (int32_t)c->n_owned, grav_mode, grav, rec);
    } else {
        auto k = c->packed_list ? force_terms_kernel<TBLOCK, true> : force_terms_kernel<TBLOCK, false>;
        k<<<grid, block, lds, st>>>(pc, c->frec, c->nlist, c->nl_cap, c->ncount, c->wave_max, c->dw_tab, c->sink, n, c->orig,
                                    (int32_t)c->n_owned, c->plan_f, grav_mode, grav, rec);
    }
    SPH_HIP(hipGetLastError());
    SPH_HIP(ensure_inv(c));
    terms_rows<<<dim3(blocks(n, 256)), dim3(256), 0, st>>>(rec, c->inv, n, d_out);
    SPH_HIP(hipGetLastError());
    if (!host) return SPH_OK;
    SPH_HIP(hipMemcpyAsync(out, d_out, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    return SPH_OK;
}

}  // namespace sph
