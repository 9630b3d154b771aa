// gradients.hip -- SPH gradients of up to four per-particle fields at the owned gas particles, in the standard (difference)
// form or the matrix-corrected form that is exact for linear fields (include/summersph.h, sph_gradients).
//
// Not part of the step loop: nothing here reads or writes the context's grid, cell table, neighbour list, statistics or
// flags.  The scratch is the one the analysis calls share (analysis_scratch).
//
// Pipeline (all on ctx->stream; counts, box and cell edge stay on the device):
//   grad_select   every slot: source (a live gas slot with a finite position) and target (a source with original id <
//                 n_owned strictly inside the clip) flags; per-block source box, source and target counts and bad-h partials;
//                 with per-particle h, an integer-atomic histogram of the sources' h by quarter octave (exponent and two
//                 mantissa bits: order-free)
//   grad_box      one wavefront: box, counts -> the cell edge E = 2 h (1 + 1e-6) for one h, 2 h_ref (1 + 1e-6) with h_ref the
//                 upper edge of the quarter octave that holds the median source; enlarged where an axis would need more than
//                 2^21 - 8 cells.  A bad target h empties the target set and marks the counts -1.
//   grad_keys     every slot: the 63-bit cell key cx << 42 | cy << 21 | cz (source) or ~0, stored at the ORIGINAL id with the
//                 slot as value, so that the stable radix sort leaves every cell in id order whatever the slot order
//   rocprim radix sort (cell key, slot)
//   grad_gather   sorted position p < sources: {x, y, z, m}, the K field values, the original id and the target flag; the first
//                 position of every cell puts {key, start} into an open-addressing hash table (atomicCAS on the key)
//   grad_tails    the last position of every cell writes its end into the cell's entry
//   rocprim select: the sorted positions of the targets, in (cell, id) order
//   grad_walk<K, CORRECTED>  one lane per target: the cells within ceil(2 h_i / E) of its own (clamped to the source box) in
//                 increasing key, each cell's sources in increasing id; rho~, C (corrected form) and b in registers; the
//                 epilogue solves and stores the rows at the original id.  Singular targets are counted with an integer atomic.
// A target's row depends only on the sources, E and the target itself: no float atomics anywhere.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "cell_table.hpp"

// the per-pair and per-target arithmetic is written in one documented order (summersph.h); no contraction into fused
// multiply-adds, so that the numpy restatement (tests/gradients_ref.py) reproduces it closely
#pragma clang fp contract(off)

namespace sph {

namespace {

constexpr int GB = 256;                    // block of the per-slot and walk kernels
constexpr int BOX_BLOCKS = 1024;           // select blocks at most (grid-stride beyond)
constexpr int NBP = 9;                     // box partials: lo (3), hi (3), sources, targets, bad
constexpr int HBINS = 8192;                // quarter octaves of a positive double: bits >> 50
constexpr double PI_DP = 3.14159265358979323846;

struct Sel {
    double clip_lo[3], clip_hi[3];
    double h_one;                          // > 0: h of every target (desc.h or a fixed-h context's params.h)
    const double *hf;                      // SPH_F_H when h_one == 0, else null
    int64_t n_owned, dead_below;
};

// on the device, written by grad_box (n_sing by grad_walk)
struct Info {
    double lo[3];
    double inv_e;                          // 1 / cell edge
    int64_t cmax[3];                       // largest cell index per axis (the source box)
    int64_t n_src;                         // sources (sorted positions [0, n_src))
    int64_t counts[2];                     // targets (-1: a target has a bad h), singular targets
    int32_t bad;
};

// the fields read: ptr[k] is a context field in slot order (by_id 0) or a row of the caller's values by original id
struct Vals {
    const double *ptr[SPH_GRAD_MAX_FIELDS];
    int32_t by_id[SPH_GRAD_MAX_FIELDS];
};

__device__ __forceinline__ bool finite3(double x, double y, double z) {
    return fabs(x) <= 1.7976931348623157e308 && fabs(y) <= 1.7976931348623157e308 && fabs(z) <= 1.7976931348623157e308;
}

__device__ __forceinline__ bool inside(const Sel &s, double x, double y, double z) {
    return s.clip_lo[0] < x && x < s.clip_hi[0] && s.clip_lo[1] < y && y < s.clip_hi[1] && s.clip_lo[2] < z && z < s.clip_hi[2];
}

__device__ __forceinline__ bool live(const Sel &s, int64_t i, int32_t id) { return !(i < s.dead_below && id >= s.n_owned); }

__device__ __forceinline__ double h_of(const Sel &s, int64_t i) { return s.h_one > 0.0 ? s.h_one : s.hf[i]; }

__device__ __forceinline__ bool good_h(double h) { return h > 0.0 && h <= 1.7976931348623157e308; }

// per-block partials lo (3), hi (3), sources, targets, bad; the h histogram (hist non-null: per-particle h)
__global__ __launch_bounds__(GB) void grad_select(const double *__restrict__ x, const double *__restrict__ y,
                                                  const double *__restrict__ z, const int32_t *__restrict__ orig, int64_t n_slots,
                                                  Sel s, double *__restrict__ part, uint32_t *__restrict__ hist) {
    __shared__ double red[NBP][GB];
    __shared__ uint32_t lh[HBINS];
    if (hist)
        for (int b = threadIdx.x; b < HBINS; b += GB) lh[b] = 0;
    __syncthreads();
    double v[NBP] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * GB) {
        const int32_t id = orig[i];
        if (!live(s, i, id)) continue;                  // replaced ghosts of a pending swap
        const double px = x[i], py = y[i], pz = z[i];
        if (!finite3(px, py, pz)) continue;
        v[0] = fmin(v[0], px); v[1] = fmin(v[1], py); v[2] = fmin(v[2], pz);
        v[3] = fmax(v[3], px); v[4] = fmax(v[4], py); v[5] = fmax(v[5], pz);
        v[6] += 1.0;
        const double h = h_of(s, i);
        if (hist && good_h(h)) atomicAdd(&lh[(uint32_t)((uint64_t)__double_as_longlong(h) >> 50)], 1u);
        if (id < s.n_owned && inside(s, px, py, pz)) {
            v[7] += 1.0;
            if (!good_h(h)) v[8] = 1.0;
        }
    }
    for (int a = 0; a < NBP; a++) red[a][threadIdx.x] = v[a];
    __syncthreads();
    for (int w = GB / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            for (int a = 0; a < 3; a++) red[a][threadIdx.x] = fmin(red[a][threadIdx.x], red[a][threadIdx.x + w]);
            for (int a = 3; a < 6; a++) red[a][threadIdx.x] = fmax(red[a][threadIdx.x], red[a][threadIdx.x + w]);
            red[6][threadIdx.x] += red[6][threadIdx.x + w];     // integer counts: exact in any order
            red[7][threadIdx.x] += red[7][threadIdx.x + w];
            red[8][threadIdx.x] = fmax(red[8][threadIdx.x], red[8][threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x < NBP) part[blockIdx.x * NBP + threadIdx.x] = red[threadIdx.x][0];
    if (hist)
        for (int b = threadIdx.x; b < HBINS; b += GB)
            if (lh[b]) atomicAdd(&hist[b], lh[b]);
}

// one wavefront: the partials (and the histogram) -> Info
__global__ __launch_bounds__(WAVE) void grad_box(const double *__restrict__ part, int nb, const uint32_t *__restrict__ hist,
                                                 double h_one, Info *__restrict__ info) {
    const int lane = threadIdx.x;
    double v[NBP] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0, 0.0, 0.0};
    for (int b = lane; b < nb; b += WAVE) {
        for (int a = 0; a < 3; a++) v[a] = fmin(v[a], part[b * NBP + a]);
        for (int a = 3; a < 6; a++) v[a] = fmax(v[a], part[b * NBP + a]);
        v[6] += part[b * NBP + 6];
        v[7] += part[b * NBP + 7];
        v[8] = fmax(v[8], part[b * NBP + 8]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        for (int a = 0; a < 3; a++) v[a] = fmin(v[a], __shfl_xor(v[a], o, 64));
        for (int a = 3; a < 6; a++) v[a] = fmax(v[a], __shfl_xor(v[a], o, 64));
        v[6] += __shfl_xor(v[6], o, 64);
        v[7] += __shfl_xor(v[7], o, 64);
        v[8] = fmax(v[8], __shfl_xor(v[8], o, 64));
    }
    // the median source's quarter octave: lane l holds bins [128 l, 128 l + 128)
    double h_ref = h_one;
    if (hist) {
        constexpr int PER = HBINS / WAVE;
        uint64_t own = 0;
        for (int b = 0; b < PER; b++) own += hist[lane * PER + b];
        uint64_t incl = own;                                // inclusive prefix over the lanes
        for (int o = 1; o < WAVE; o <<= 1) {
            const uint64_t t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        const uint64_t total = __shfl(incl, WAVE - 1, 64);
        h_ref = 0.0;
        if (total > 0) {
            const uint64_t rank = (total - 1) / 2;          // the lower median
            const uint64_t before = incl - own;
            int bin = -1;
            if (rank >= before && rank < incl) {
                uint64_t acc = before;
                for (int b = 0; b < PER; b++) {
                    acc += hist[lane * PER + b];
                    if (rank < acc) { bin = lane * PER + b; break; }
                }
            }
            for (int o = 32; o > 0; o >>= 1) bin = max(bin, __shfl_xor(bin, o, 64));
            h_ref = __longlong_as_double((long long)((uint64_t)(bin + 1) << 50));     // the bin's upper edge
        }
    }
    if (lane != 0) return;
    const bool empty = !(v[6] > 0.0);
    double e = (2.0 * h_ref) * (1.0 + 1e-6);
    if (!(e > 0.0 && e <= 1.7976931348623157e308)) e = 1.0;    // no usable h: any edge serves (bad h, no source)
    for (int a = 0; a < 3; a++) {
        const double ext = empty ? 0.0 : v[3 + a] - v[a];
        if (ext / e > AXIS_CELLS) e = (ext / AXIS_CELLS) * (1.0 + 1e-6);
    }
    const double ie = 1.0 / e;
    const bool bad = v[8] != 0.0;
    for (int a = 0; a < 3; a++) {
        const double lo = empty ? 0.0 : v[a];
        info->lo[a] = lo;
        info->cmax[a] = empty ? 0 : (int64_t)fmin(fmax(floor((v[3 + a] - lo) * ie), 0.0), (double)AXIS_MASK);
    }
    info->inv_e = ie;
    info->n_src = empty ? 0 : (int64_t)v[6];
    info->counts[0] = bad ? -1 : (int64_t)v[7];
    info->counts[1] = 0;
    info->bad = bad ? 1 : 0;
}

// keys[id] = the cell key of a source (~0 otherwise), vals[id] = its slot
__global__ __launch_bounds__(GB) void grad_keys(const double *__restrict__ x, const double *__restrict__ y,
                                                const double *__restrict__ z, const int32_t *__restrict__ orig, int64_t n_slots,
                                                Sel s, const Info *__restrict__ info, uint64_t *__restrict__ keys,
                                                uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (i >= n_slots) return;
    const int32_t id = orig[i];
    if (!live(s, i, id)) return;
    const double px = x[i], py = y[i], pz = z[i];
    uint64_t key = ~0ull;
    if (finite3(px, py, pz)) key = cell_key(px, py, pz, info->lo, info->inv_e);
    keys[id] = key;
    vals[id] = (uint32_t)i;
}

// {x, y, z, m}, the values (stride KS), the original id and the target flag in sorted order; every cell's first position
// enters the table
__global__ __launch_bounds__(GB) void grad_gather(const double *__restrict__ x, const double *__restrict__ y,
                                                  const double *__restrict__ z, const double *__restrict__ m,
                                                  const int32_t *__restrict__ orig, Sel s, Vals vf, int nf, int ks,
                                                  const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sval,
                                                  const Info *__restrict__ info, int64_t n, double4 *__restrict__ rec,
                                                  double *__restrict__ av, int32_t *__restrict__ sid, uint8_t *__restrict__ tflag,
                                                  Ent *__restrict__ tab, uint64_t mask) {
    const int64_t p = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (p >= n || p >= info->n_src) return;
    const uint32_t i = sval[p];
    const int32_t id = orig[i];
    const double px = x[i], py = y[i], pz = z[i];
    rec[p] = make_double4(px, py, pz, m[i]);
    for (int k = 0; k < nf; k++) av[p * ks + k] = vf.by_id[k] ? vf.ptr[k][id] : vf.ptr[k][i];
    sid[p] = id;
    tflag[p] = (info->bad == 0 && id < s.n_owned && inside(s, px, py, pz)) ? 1 : 0;
    cell_enter(skey, p, tab, mask);
}

__global__ __launch_bounds__(GB) void grad_tails(const uint64_t *__restrict__ skey, const Info *__restrict__ info, int64_t n,
                                                 Ent *__restrict__ tab, uint64_t mask) {
    cell_close(skey, (int64_t)blockIdx.x * GB + threadIdx.x, n, info->n_src, tab, mask);
}

// one lane per target (t-th target in sorted order: sorted position tlist[t])
template <int K, bool CORRECTED>
__global__ __launch_bounds__(GB) void grad_walk(const double4 *__restrict__ rec, const double *__restrict__ av,
                                                const int32_t *__restrict__ sid, const uint64_t *__restrict__ skey,
                                                const uint32_t *__restrict__ sval, const int32_t *__restrict__ tlist,
                                                Info *__restrict__ info, int64_t n, const Ent *__restrict__ tab, uint64_t mask,
                                                double h_one, const double *__restrict__ hf, double *__restrict__ out,
                                                double *__restrict__ rho_out) {
    constexpr int KS = K == 3 ? 4 : K;
    const int64_t t = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (t >= n || t >= info->counts[0]) return;            // counts[0] == -1 (bad h): no target
    const int64_t p = tlist[t];
    const double4 r = rec[p];
    const double h = h_one > 0.0 ? h_one : hf[sval[p]];
    double ai[K];
#pragma unroll
    for (int k = 0; k < K; k++) ai[k] = av[p * KS + k];
    const uint64_t key = skey[p];
    const int64_t c[3] = {(int64_t)(key >> (2 * AXIS_BITS)), (int64_t)((key >> AXIS_BITS) & AXIS_MASK), (int64_t)(key & AXIS_MASK)};
    // ceil(2 h / E) cells either way (the 1e-7 covers the rounding of the cell coordinates), clamped to the source box
    const double reach = ceil((2.0 * h) * info->inv_e + 1e-7);
    int64_t lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        const double cm = (double)info->cmax[a];
        lo[a] = (int64_t)fmax((double)c[a] - reach, 0.0);
        hi[a] = (int64_t)fmin((double)c[a] + reach, cm);
    }
    const double r2max = 4.0 * (h * h), ih = 1.0 / h;
    double sw = 0.0, cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
    double bx[K], by[K], bz[K];
#pragma unroll
    for (int k = 0; k < K; k++) { bx[k] = 0.0; by[k] = 0.0; bz[k] = 0.0; }
    for (int64_t n0 = lo[0]; n0 <= hi[0]; n0++)
        for (int64_t n1 = lo[1]; n1 <= hi[1]; n1++)
            for (int64_t n2 = lo[2]; n2 <= hi[2]; n2++) {
                const uint64_t nk = ((uint64_t)n0 << (2 * AXIS_BITS)) | ((uint64_t)n1 << AXIS_BITS) | (uint64_t)n2;
                const int64_t e = hash_slot(tab, mask, nk);
                if (e < 0) continue;
                const int32_t q0 = tab[e].start, q1 = tab[e].end;
                for (int32_t q = q0; q < q1; q++) {
                    const double4 s = rec[q];
                    const double dx = r.x - s.x, dy = r.y - s.y, dz = r.z - s.z;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (!(d2 <= r2max)) continue;
                    const double qq = sqrt(d2) * ih;
                    const double tq = 2.0 - qq;
                    const double w = qq <= 1.0 ? (1.0 - 1.5 * (qq * qq)) + 0.75 * ((qq * qq) * qq) : 0.25 * ((tq * tq) * tq);
                    sw += s.w * w;
                    if (d2 == 0.0) continue;                   // the target itself and coincident particles: nothing to C, b
                    const double f = qq <= 1.0 ? 3.0 - 2.25 * qq : (0.75 * (tq * tq)) / qq;
                    const double mf = s.w * f;
                    if (CORRECTED) {
                        const double fx = mf * dx, fy = mf * dy;
                        cxx += fx * dx; cxy += fx * dy; cxz += fx * dz;
                        cyy += fy * dy; cyz += fy * dz; czz += (mf * dz) * dz;
                    }
#pragma unroll
                    for (int k = 0; k < K; k++) {
                        const double g = mf * (ai[k] - av[(int64_t)q * KS + k]);
                        bx[k] += g * dx; by[k] += g * dy; bz[k] += g * dz;
                    }
                }
            }
    const int32_t id = sid[p];
    const double sig = 1.0 / (PI_DP * ((h * h) * h));
    const double rho = sig * sw;
    if (rho_out) rho_out[id] = rho;
    if (CORRECTED) {
        // adj(C) b / det C; C symmetric {cxx cxy cxz; cxy cyy cyz; cxz cyz czz}
        const double a00 = cyy * czz - cyz * cyz, a01 = cxz * cyz - cxy * czz, a02 = cxy * cyz - cxz * cyy;
        const double a11 = cxx * czz - cxz * cxz, a12 = cxy * cxz - cxx * cyz, a22 = cxx * cyy - cxy * cxy;
        const double det = (cxx * a00 + cxy * a01) + cxz * a02;
        const double t3 = ((cxx + cyy) + czz) / 3.0;
        const bool singular = !(det > 1e-6 * ((t3 * t3) * t3));
        if (singular) atomicAdd(reinterpret_cast<unsigned long long *>(&info->counts[1]), 1ull);
#pragma unroll
        for (int k = 0; k < K; k++) {
            double g[3] = {NAN, NAN, NAN};
            if (!singular) {
                g[0] = ((a00 * bx[k] + a01 * by[k]) + a02 * bz[k]) / det;
                g[1] = ((a01 * bx[k] + a11 * by[k]) + a12 * bz[k]) / det;
                g[2] = ((a02 * bx[k] + a12 * by[k]) + a22 * bz[k]) / det;
            }
            for (int a = 0; a < 3; a++) out[(3 * k + a) * n + id] = g[a];
        }
    } else {
        const double sc = sig / (h * h);               // F = (sigma / h^2) f
#pragma unroll
        for (int k = 0; k < K; k++) {
            out[(3 * k + 0) * n + id] = (sc * bx[k]) / rho;
            out[(3 * k + 1) * n + id] = (sc * by[k]) / rho;
            out[(3 * k + 2) * n + id] = (sc * bz[k]) / rho;
        }
    }
}

template <int K>
hipError_t launch_walk(bool corrected, unsigned nb, hipStream_t st, const double4 *rec, const double *av, const int32_t *sid,
                       const uint64_t *skey, const uint32_t *sval, const int32_t *tlist, Info *info, int64_t n, const Ent *tab,
                       uint64_t mask, double h_one, const double *hf, double *out, double *rho_out) {
    if (corrected)
        grad_walk<K, true><<<dim3(nb), dim3(GB), 0, st>>>(rec, av, sid, skey, sval, tlist, info, n, tab, mask, h_one, hf, out, rho_out);
    else
        grad_walk<K, false><<<dim3(nb), dim3(GB), 0, st>>>(rec, av, sid, skey, sval, tlist, info, n, tab, mask, h_one, hf, out, rho_out);
    return hipGetLastError();
}

}  // namespace

int gradients_run(sph_ctx *c, const sph_gradients_desc *d, const double *values, double *out, int64_t n_out, double *rho_out,
                  int64_t *counts, bool host) {
    const char *who = "sph_gradients";
    if (!d) return arg_error(c, who, "null descriptor");
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return arg_error(c, who, "reserved must be 0");
    if (d->flags & ~SPH_GRAD_CORRECTED) return arg_error(c, who, "unknown flags");
    const int nf = d->n_fields;
    if (nf < 1 || nf > SPH_GRAD_MAX_FIELDS) return arg_error(c, who, "n_fields must be 1 .. SPH_GRAD_MAX_FIELDS");
    bool any_values = false;
    for (int k = 0; k < nf; k++) {
        if (d->fields[k] != SPH_GRAD_VALUES && (d->fields[k] < 0 || d->fields[k] >= SPH_F_COUNT))
            return arg_error(c, who, "field id out of range");
        any_values = any_values || d->fields[k] == SPH_GRAD_VALUES;
    }
    if (any_values != (values != nullptr)) return arg_error(c, who, "values must be given with SPH_GRAD_VALUES and only then");
    const int64_t n = c->n;
    if (n_out != 3 * (int64_t)nf * n) return arg_error(c, who, "n_out != 3 n_fields sph_count");
    if (!out && n_out > 0) return arg_error(c, who, "null output");
    if (std::isnan(d->h) || d->h < 0.0) return arg_error(c, who, "h must be >= 0");
    for (int a = 0; a < 3; a++)
        if (std::isnan(d->clip_lo[a]) || std::isnan(d->clip_hi[a])) return arg_error(c, who, "the clip box has a NaN");
    for (int k = 0; k < nf; k++)
        if (d->fields[k] >= 0 && !field_ready(*c, c->variable, d->fields[k])) {
            c->err = "sph_gradients: a field is stale (as sph_download_field would refuse it)";
            return SPH_ERR_STATE;
        }
    const bool per_particle = !(d->h > 0.0) && c->variable;
    const double h_one = d->h > 0.0 ? d->h : (c->variable ? 0.0 : c->p.h);
    if (!per_particle && !(h_one > 0.0)) {
        c->err = "sph_gradients: params.h <= 0 on a fixed-h context (give desc.h > 0)";
        return SPH_ERR_STATE;
    }
    const bool corrected = (d->flags & SPH_GRAD_CORRECTED) != 0;

    hipStream_t st = c->stream;
    const int64_t ns = c->cap > 0 ? c->n_slots : 0;
    if (ns == 0 || n == 0) {                        // nothing held: no target
        if (host) {
            if (counts) { counts[0] = 0; counts[1] = 0; }
        } else if (counts) {
            SPH_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
        }
        return SPH_OK;
    }
    const int ks = nf == 3 ? 4 : nf;                             // value stride of the sorted records
    const int nb = (int)std::min<int64_t>((ns + GB - 1) / GB, BOX_BLOCKS);
    int64_t tl = 1;
    while (tl < 2 * n) tl <<= 1;                                 // hash table: load <= 1/2
    size_t sort_bytes = 0, select_bytes = 0;
    SPH_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)n, 0u, 64u, st));
    SPH_HIP(rocprim::select(nullptr, select_bytes, rocprim::counting_iterator<int32_t>(0), (const uint8_t *)nullptr,
                            (int32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, st));
    uint64_t *keys, *keys_alt;
    uint32_t *vals, *vals_alt, *sel_count, *hist_buf;
    char *sort_tmp, *select_tmp;
    double4 *rec;
    Ent *tab;
    Info *info;
    int32_t *sid, *tlist;
    uint8_t *tflag;
    double *av, *box_part, *h_values, *h_out, *h_rho;
    auto layout = [&](Carve cv) {
        keys = cv.take<uint64_t>(n);
        keys_alt = cv.take<uint64_t>(n);
        vals = cv.take<uint32_t>(n);
        vals_alt = cv.take<uint32_t>(n);
        sort_tmp = cv.take<char>(sort_bytes);
        select_tmp = cv.take<char>(select_bytes);
        rec = cv.take<double4>(n);
        av = cv.take<double>((size_t)ks * (size_t)n);
        sid = cv.take<int32_t>(n);
        tflag = cv.take<uint8_t>(n);
        tlist = cv.take<int32_t>(n);
        sel_count = cv.take<uint32_t>(1);
        tab = cv.take<Ent>(tl);
        box_part = cv.take<double>(NBP * (size_t)nb);
        hist_buf = cv.take<uint32_t>(per_particle ? HBINS : 0);
        info = cv.take<Info>(1);
        h_values = cv.take<double>(host && values ? (size_t)nf * (size_t)n : 0);     // the host form's device copies
        h_out = cv.take<double>(host ? n_out : 0);
        h_rho = cv.take<double>(host && rho_out ? n : 0);
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    uint32_t *hist = per_particle ? hist_buf : nullptr;
    const double *d_values = host && values ? h_values : values;
    double *d_out = host ? h_out : out;
    double *d_rho = host ? (rho_out ? h_rho : nullptr) : rho_out;
    if (host) SPH_TRY(analysis_pinned(c));

    Sel s{};
    for (int a = 0; a < 3; a++) { s.clip_lo[a] = d->clip_lo[a]; s.clip_hi[a] = d->clip_hi[a]; }
    s.h_one = h_one;
    s.hf = per_particle ? c->f[SPH_F_H] : nullptr;
    s.n_owned = c->n_owned;
    s.dead_below = c->dead_below;
    Vals vf{};
    for (int k = 0; k < nf; k++) {
        const bool by_id = d->fields[k] == SPH_GRAD_VALUES;
        vf.by_id[k] = by_id ? 1 : 0;
        vf.ptr[k] = by_id ? d_values + (size_t)k * (size_t)n : c->f[d->fields[k]];
        if (by_id && host) SPH_HIP(hipMemcpyAsync(const_cast<double *>(vf.ptr[k]), values + (size_t)k * (size_t)n,
                                                  (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    }
    const double *x = c->f[SPH_F_X], *y = c->f[SPH_F_Y], *z = c->f[SPH_F_Z];

    // every row NaN until its target writes it
    SPH_HIP(hipMemsetAsync(d_out, 0xff, (size_t)n_out * sizeof(double), st));
    if (d_rho) SPH_HIP(hipMemsetAsync(d_rho, 0xff, (size_t)n * sizeof(double), st));
    // selection, box, cell edge
    if (hist) SPH_HIP(hipMemsetAsync(hist, 0, 4 * (size_t)HBINS, st));
    grad_select<<<dim3((unsigned)nb), dim3(GB), 0, st>>>(x, y, z, c->orig, ns, s, box_part, hist);
    grad_box<<<dim3(1), dim3(WAVE), 0, st>>>(box_part, nb, hist, h_one, info);
    SPH_HIP(hipGetLastError());
    // cell keys by original id, sort, hash table over the occupied cells
    grad_keys<<<dim3(blocks(ns, GB)), dim3(GB), 0, st>>>(x, y, z, c->orig, ns, s, info, keys, vals);
    size_t tmp = sort_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, keys, keys_alt, vals, vals_alt, (size_t)n, 0u, 64u, st));
    SPH_HIP(hipMemsetAsync(tab, 0xff, sizeof(Ent) * (size_t)tl, st));
    SPH_HIP(hipMemsetAsync(tflag, 0, (size_t)n, st));
    grad_gather<<<dim3(blocks(n, GB)), dim3(GB), 0, st>>>(x, y, z, c->f[SPH_F_M], c->orig, s, vf, nf, ks, keys_alt, vals_alt,
                                                           info, n, rec, av, sid, tflag, tab, (uint64_t)(tl - 1));
    grad_tails<<<dim3(blocks(n, GB)), dim3(GB), 0, st>>>(keys_alt, info, n, tab, (uint64_t)(tl - 1));
    SPH_HIP(hipGetLastError());
    // the targets in sorted order
    tmp = select_bytes;
    SPH_HIP(rocprim::select(select_tmp, tmp, rocprim::counting_iterator<int32_t>(0), (const uint8_t *)tflag, tlist, sel_count,
                            (size_t)n, st));
    const unsigned wb = blocks(n, GB);
    hipError_t e = hipSuccess;
    switch (nf) {
        case 1: e = launch_walk<1>(corrected, wb, st, rec, av, sid, keys_alt, vals_alt, tlist, info, n, tab, (uint64_t)(tl - 1), h_one, s.hf, d_out, d_rho); break;
        case 2: e = launch_walk<2>(corrected, wb, st, rec, av, sid, keys_alt, vals_alt, tlist, info, n, tab, (uint64_t)(tl - 1), h_one, s.hf, d_out, d_rho); break;
        case 3: e = launch_walk<3>(corrected, wb, st, rec, av, sid, keys_alt, vals_alt, tlist, info, n, tab, (uint64_t)(tl - 1), h_one, s.hf, d_out, d_rho); break;
        default: e = launch_walk<4>(corrected, wb, st, rec, av, sid, keys_alt, vals_alt, tlist, info, n, tab, (uint64_t)(tl - 1), h_one, s.hf, d_out, d_rho); break;
    }
    SPH_HIP(e);
    if (!host) {
        if (counts) SPH_HIP(hipMemcpyAsync(counts, info->counts, 2 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        return SPH_OK;
    }
    // host form: the counts, the rows and rho~ in one read-back
    SPH_HIP(hipMemcpyAsync(c->rnd_pinned, info->counts, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipMemcpyAsync(out, d_out, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    if (rho_out) SPH_HIP(hipMemcpyAsync(rho_out, d_rho, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    int64_t cnt[2] = {0, 0};
    std::memcpy(cnt, c->rnd_pinned, sizeof(cnt));
    if (cnt[0] < 0) {
        c->err = "sph_gradients: a target has h <= 0 or a non-finite h";
        return SPH_ERR_STATE;
    }
    if (counts) { counts[0] = cnt[0]; counts[1] = cnt[1]; }
    return SPH_OK;
}

}  // namespace sph
