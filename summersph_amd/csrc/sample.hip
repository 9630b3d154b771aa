// sample.hip -- the SPH interpolant at arbitrary points: den(p) = sum_j ws_j Wn(|p - r_j| / h_j) and up to four
// num_k(p) = sum_j (ws_j A_j^(k)) Wn(...) over the owned gas, in scatter form (every source with its own h_j) at points
// that have no h of their own (include/summersph.h, sph_sample).
//
// Not part of the step loop: nothing here reads or writes the context's grid, cell table, neighbour list, statistics or
// flags.  The scratch is the one the analysis calls share (analysis_scratch).
//
// A point must find every source j with |p - r_j| <= 2 h_j when h_j varies by octaves.  The sources are therefore binned
// by LEVELS of h: level l holds the sources with h in (H_{l-1}, H_l] in a cell grid of edge E_l = 2 H_l (1 + 1e-6) over the
// common source box, so that the 3 x 3 x 3 cells of level l around a point hold every level-l source that can reach it.
// All levels live in one sorted record sequence and one hashed cell table (cell_table.hpp, level-aware keys).
//
// Pipeline (all on ctx->stream; counts, box, levels and cell edges stay on the device):
//   sample_select   every slot: source (owned gas strictly inside the clip box); per-block source box, count and bad-h
//                   partials; with per-particle h an integer-atomic histogram of the sources' h by quarter octave
//   sample_levels   one wavefront: box, count, the occupied levels (aligned groups of 2^g quarter octaves; g grows until
//                   at most 64 levels are occupied -- merging upwards is always valid, a smaller h in a larger cell is
//                   still found), every level's edge (enlarged where an axis would need more than 2^19 - 8 cells) and the
//                   most populated level
//   sample_keys     every slot: the 63-bit key level << 57 | cx << 38 | cy << 19 | cz (source) or ~0, stored at the ORIGINAL
//                   id with the slot as value, so that the stable radix sort leaves (level, cell, id) order whatever the
//                   slot order
//   rocprim radix sort (key, slot)
//   sample_records  sorted position p < sources: {x, y, z, 1 / h_j} and {ws_j, ws_j A_j^(0..K-1)}; the first position of
//                   every cell puts {key, start} into the hash table
//   sample_tails    the last position of every cell writes its end
//   sample_point_keys + rocprim radix sort   the points by their cell in the most populated level (index as value): the
//                   64 lanes of a wavefront then walk neighbouring cells.  Only the work distribution depends on it.
//   sample_walk<K, PER_H>   one lane per point: the levels in ascending order, in each the <= 27 cells around the point's
//                   (signed, unclamped) cell that lie inside the source box, in ascending key, skipping a cell whose
//                   nearest face is farther than 2 H_l; each cell's records in id order; den and the K num in registers.
//                   Epilogue: normalise, store at the point's original index, integer-atomic counts.
// A point's values depend only on the sources, the descriptor and the point itself: no float atomics anywhere.
//
// The steps up to sample_tails are sample_build, which sph_trace (trace.hip) calls too; what its walk shares with sample_walk
// on the device (Level, Info, kernel_w, add_range, point_sums: the level / cell loop of a point) is in sample_common.hpp.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

// the per-pair arithmetic is written in one documented order (summersph.h); no contraction into fused multiply-adds
#pragma clang fp contract(off)

#include "sample_common.hpp"

namespace sph {

namespace {

constexpr int SB = 256;                    // block of the per-slot, per-point and walk kernels
constexpr int BOX_BLOCKS = 1024;           // select blocks at most (grid-stride beyond)
constexpr int NBP = 8;                     // box partials: lo (3), hi (3), sources, bad
constexpr int HBINS = SAMPLE_HBINS;
constexpr int HSHIFT = 50;
constexpr double DBL_BIG = SAMPLE_DBL_BIG;

struct Sel {
    double clip_lo[3], clip_hi[3];
    double h_one;                          // > 0: h of every source (desc.h or a fixed-h context's params.h)
    const double *hf;                      // SPH_F_H when h_one == 0, else null
    int64_t n_owned;
};

// the fields read: ptr[k] is a context field in slot order (by_id 0) or a row of the caller's values by original id
struct Vals {
    const double *ptr[SPH_SAMPLE_MAX_FIELDS];
    int32_t by_id[SPH_SAMPLE_MAX_FIELDS];
};

// the renders' selection: owned, strictly inside the clip box (a non-finite position is never inside)
__device__ __forceinline__ bool source(const Sel &s, int32_t id, double x, double y, double z) {
    return id < s.n_owned && s.clip_lo[0] < x && x < s.clip_hi[0] && s.clip_lo[1] < y && y < s.clip_hi[1] &&
           s.clip_lo[2] < z && z < s.clip_hi[2];
}

__device__ __forceinline__ double h_of(const Sel &s, int64_t i) { return s.h_one > 0.0 ? s.h_one : s.hf[i]; }

__device__ __forceinline__ bool good_h(double h) { return h > 0.0 && h <= DBL_BIG; }

// per-block partials lo (3), hi (3), sources, bad; the h histogram (hist non-null: per-particle h)
__global__ __launch_bounds__(SB) void sample_select(const double *__restrict__ x, const double *__restrict__ y,
                                                    const double *__restrict__ z, const int32_t *__restrict__ orig,
                                                    int64_t n_slots, Sel s, double *__restrict__ part,
                                                    uint32_t *__restrict__ hist) {
    __shared__ double red[NBP][SB];
    __shared__ uint32_t lh[HBINS];
    if (hist)
        for (int b = threadIdx.x; b < HBINS; b += SB) lh[b] = 0;
    __syncthreads();
    double v[NBP] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * SB) {
        const double px = x[i], py = y[i], pz = z[i];
        if (!source(s, orig[i], px, py, pz)) continue;
        v[0] = fmin(v[0], px); v[1] = fmin(v[1], py); v[2] = fmin(v[2], pz);
        v[3] = fmax(v[3], px); v[4] = fmax(v[4], py); v[5] = fmax(v[5], pz);
        v[6] += 1.0;
        const double h = h_of(s, i);
        if (!good_h(h)) v[7] = 1.0;
        else if (hist) atomicAdd(&lh[(uint32_t)((uint64_t)__double_as_longlong(h) >> HSHIFT)], 1u);
    }
    for (int a = 0; a < NBP; a++) red[a][threadIdx.x] = v[a];
    __syncthreads();
    for (int w = SB / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            for (int a = 0; a < 3; a++) red[a][threadIdx.x] = fmin(red[a][threadIdx.x], red[a][threadIdx.x + w]);
            for (int a = 3; a < 6; a++) red[a][threadIdx.x] = fmax(red[a][threadIdx.x], red[a][threadIdx.x + w]);
            red[6][threadIdx.x] += red[6][threadIdx.x + w];     // integer counts: exact in any order
            red[7][threadIdx.x] = fmax(red[7][threadIdx.x], red[7][threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x < NBP) part[blockIdx.x * NBP + threadIdx.x] = red[threadIdx.x][0];
    if (hist)
        for (int b = threadIdx.x; b < HBINS; b += SB)
            if (lh[b]) atomicAdd(&hist[b], lh[b]);
}

// level l of upper smoothing length H over a box of extent ext
__device__ __forceinline__ void set_level(Level &L, double H, const double *ext) {
    double e = (2.0 * H) * (1.0 + 1e-6);
    if (!(e > 0.0 && e <= DBL_BIG)) e = DBL_BIG;
    for (int a = 0; a < 3; a++)
        if (ext[a] / e > LEVEL_AXIS_CELLS) e = (ext[a] / LEVEL_AXIS_CELLS) * (1.0 + 1e-6);
    const double ie = 1.0 / e;
    L.edge = e;
    L.inv_e = ie;
    L.cull2 = ((2.0 * H) * (2.0 * H)) * (1.0 + 1e-5);       // overflows to +inf for a huge H: no cell is skipped then
    for (int a = 0; a < 3; a++) L.cmax[a] = (int32_t)fmin(fmax(floor(ext[a] * ie), 0.0), (double)LEVEL_AXIS_MASK);
    L.pad = 0;
}

// one wavefront: the partials (and the histogram) -> Info.  g0: the narrowest level width tried (2^g0 quarter octaves).
__global__ __launch_bounds__(WAVE) void sample_levels(const double *__restrict__ part, int nb, const uint32_t *__restrict__ hist,
                                                      double h_one, int g0, Info *__restrict__ info) {
    const int lane = threadIdx.x;
    double v[NBP] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0, 0.0};
    for (int b = lane; b < nb; b += WAVE) {
        for (int a = 0; a < 3; a++) v[a] = fmin(v[a], part[b * NBP + a]);
        for (int a = 3; a < 6; a++) v[a] = fmax(v[a], part[b * NBP + a]);
        v[6] += part[b * NBP + 6];
        v[7] = fmax(v[7], part[b * NBP + 7]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        for (int a = 0; a < 3; a++) v[a] = fmin(v[a], __shfl_xor(v[a], o, 64));
        for (int a = 3; a < 6; a++) v[a] = fmax(v[a], __shfl_xor(v[a], o, 64));
        v[6] += __shfl_xor(v[6], o, 64);
        v[7] = fmax(v[7], __shfl_xor(v[7], o, 64));
    }
    const bool bad = v[7] != 0.0;
    const bool empty = !(v[6] > 0.0) || bad;                  // a bad h empties the source set: every output is NaN
    double ext[3];
    for (int a = 0; a < 3; a++) ext[a] = empty ? 0.0 : v[3 + a] - v[a];
    int nlev = 0, top = 0, g = 0;
    if (!empty && !hist) {                                    // one h: one level
        nlev = 1;
        if (lane == 0) set_level(info->lv[0], h_one, ext);
    } else if (!empty) {
        // the level width: the smallest g >= g0 with at most MAX_LEVELS occupied groups of 2^g quarter octaves
        for (g = g0;; g++) {
            const int ng = HBINS >> g;
            int occ = 0;
            for (int cb = lane; cb < ng; cb += WAVE) {
                uint32_t any = 0;
                for (int b = cb << g; b < (cb + 1) << g; b++) any |= hist[b];
                occ += any != 0;
            }
            for (int o = 32; o > 0; o >>= 1) occ += __shfl_xor(occ, o, 64);
            if (occ <= MAX_LEVELS) { nlev = occ; break; }     // g = 13: one group, always accepted
        }
        // lane l numbers the groups [l per, l per + per) in ascending order
        const int ng = HBINS >> g;
        const int per = ng >= WAVE ? ng / WAVE : 1;
        const int c0 = lane * per, c1 = min(c0 + per, ng);
        int own = 0;
        for (int cb = c0; cb < c1; cb++) {
            uint32_t any = 0;
            for (int b = cb << g; b < (cb + 1) << g; b++) any |= hist[b];
            own += any != 0;
        }
        int incl = own;
        for (int o = 1; o < WAVE; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        int l = incl - own;
        unsigned long long best_n = 0;
        int best_l = MAX_LEVELS;
        for (int cb = c0; cb < c1; cb++) {
            unsigned long long cnt = 0;
            for (int b = cb << g; b < (cb + 1) << g; b++) cnt += hist[b];
            if (cnt == 0) continue;
            for (int b = cb << g; b < (cb + 1) << g; b++) info->level_of[b] = (uint8_t)l;
            // the group's upper edge; the last group's would be +inf
            const uint64_t bits = (uint64_t)(cb + 1) << (HSHIFT + g);
            const double H = bits >= 0x7ff0000000000000ull ? DBL_BIG : __longlong_as_double((long long)bits);
            set_level(info->lv[l], H, ext);
            if (cnt > best_n) { best_n = cnt; best_l = l; }   // ascending l: the first of equal counts stays
            l++;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long on = __shfl_xor(best_n, o, 64);
            const int ol = __shfl_xor(best_l, o, 64);
            if (on > best_n || (on == best_n && ol < best_l)) { best_n = on; best_l = ol; }
        }
        top = best_l < MAX_LEVELS ? best_l : 0;
    }
    if (lane != 0) return;
    for (int a = 0; a < 3; a++) info->lo[a] = empty ? 0.0 : v[a];
    info->n_src = empty ? 0 : (int64_t)v[6];
    info->counts[0] = bad ? -1 : 0;
    info->counts[1] = 0;
    info->bad = bad ? 1 : 0;
    info->nlev = nlev;
    info->top = top;
    info->g = g;
}

// a context that holds nothing: no source, no level
__global__ __launch_bounds__(WAVE) void sample_no_sources(Info *__restrict__ info) {
    if (threadIdx.x != 0) return;
    for (int a = 0; a < 3; a++) info->lo[a] = 0.0;
    info->n_src = 0;
    info->counts[0] = 0; info->counts[1] = 0;
    info->bad = 0; info->nlev = 0; info->top = 0; info->g = 0;
}

// keys[id] = the (level, cell) key of a source (~0 otherwise: the caller's fill), vals[id] = its slot
__global__ __launch_bounds__(SB) void sample_keys(const double *__restrict__ x, const double *__restrict__ y,
                                                  const double *__restrict__ z, const int32_t *__restrict__ orig, int64_t n_slots,
                                                  Sel s, const Info *__restrict__ info, uint64_t *__restrict__ keys,
                                                  uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (i >= n_slots || info->n_src == 0) return;
    const int32_t id = orig[i];
    const double px = x[i], py = y[i], pz = z[i];
    if (!source(s, id, px, py, pz)) return;
    const uint64_t l = s.h_one > 0.0 ? 0 : info->level_of[(uint32_t)((uint64_t)__double_as_longlong(s.hf[i]) >> HSHIFT)];
    const Level &L = info->lv[l];
    keys[id] = level_key(l, level_cell_axis(px, info->lo[0], L.inv_e, L.cmax[0]), level_cell_axis(py, info->lo[1], L.inv_e, L.cmax[1]),
                         level_cell_axis(pz, info->lo[2], L.inv_e, L.cmax[2]));
    vals[id] = (uint32_t)i;
}

// {x, y, z, 1 / h} and {ws, ws A^(0..nf-1)} (stride nf + 1) in sorted order; every cell's first position enters the table.
// s_j = 1 / (pi h_j^3), ws_j = m_j s_j (rho null) or (m_j / rho_j) s_j: the renders' record arithmetic.
__global__ __launch_bounds__(SB) void sample_records(const double *__restrict__ x, const double *__restrict__ y,
                                                     const double *__restrict__ z, const double *__restrict__ m,
                                                     const double *__restrict__ rho, const int32_t *__restrict__ orig, Sel s,
                                                     Vals vf, int nf, const uint64_t *__restrict__ skey,
                                                     const uint32_t *__restrict__ sval, const Info *__restrict__ info, int64_t n,
                                                     double4 *__restrict__ rec, double *__restrict__ wsa, Ent *__restrict__ tab,
                                                     uint64_t mask) {
    const int64_t p = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (p >= n || p >= info->n_src) return;
    const uint32_t i = sval[p];
    const int32_t id = orig[i];
    const double h = h_of(s, i);
    const double sg = 1.0 / (M_PI * (h * h * h));
    const double ws = (rho ? m[i] / rho[i] : m[i]) * sg;
    rec[p] = make_double4(x[i], y[i], z[i], 1.0 / h);
    double *w = wsa + p * (int64_t)(nf + 1);
    w[0] = ws;
    for (int k = 0; k < nf; k++) w[1 + k] = ws * (vf.by_id[k] ? vf.ptr[k][id] : vf.ptr[k][i]);
    cell_enter(skey, p, tab, mask);
}

__global__ __launch_bounds__(SB) void sample_tails(const uint64_t *__restrict__ skey, const Info *__restrict__ info, int64_t n,
                                                   Ent *__restrict__ tab, uint64_t mask) {
    cell_close(skey, (int64_t)blockIdx.x * SB + threadIdx.x, n, info->n_src, tab, mask);
}

// the points' sort keys: their (clamped) cell in the most populated level, POINT_KEY_NONE for a non-finite point
__global__ __launch_bounds__(SB) void sample_point_keys(const double *__restrict__ px, const double *__restrict__ py,
                                                        const double *__restrict__ pz, int64_t m, const Info *__restrict__ info,
                                                        uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t t = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (t >= m) return;
    keys[t] = point_sort_key(info, px[t], py[t], pz[t]);
    vals[t] = (uint32_t)t;
}

// one lane per point (the t-th in walk order: point pidx[t], or t itself without the point sort)
template <int K, bool PER_H>
__global__ __launch_bounds__(SB) void sample_walk(const double *__restrict__ px, const double *__restrict__ py,
                                                  const double *__restrict__ pz, const uint32_t *__restrict__ pidx, int64_t m,
                                                  Info *__restrict__ info, const double4 *__restrict__ rec,
                                                  const double *__restrict__ wsa, const Ent *__restrict__ tab, uint64_t mask,
                                                  double h_one, int normalise, double *__restrict__ out,
                                                  double *__restrict__ weight) {
    const int64_t t = (int64_t)blockIdx.x * SB + threadIdx.x;
    const bool active = t < m;
    const int64_t idx = active ? (pidx ? (int64_t)pidx[t] : t) : 0;
    double p[3] = {0.0, 0.0, 0.0};
    if (active) { p[0] = px[idx]; p[1] = py[idx]; p[2] = pz[idx]; }
    const bool fin = finite3(p[0], p[1], p[2]);
    const bool bad = info->bad != 0;
    double den = 0.0, num[K > 0 ? K : 1];
#pragma unroll
    for (int k = 0; k < K; k++) num[k] = 0.0;
    const int nlev = (active && fin) ? info->nlev : 0;
    const double ih_one = 1.0 / h_one;                       // one h: the records' 1 / h_j, bitwise
    point_sums<K, PER_H>(info, rec, wsa, tab, mask, nlev, p, ih_one, den, num);
    const bool nan = !fin || bad;
    if (active) {
#pragma unroll
        for (int k = 0; k < K; k++)
            out[(int64_t)k * m + idx] = nan ? NAN : (normalise ? (den != 0.0 ? num[k] / den : 0.0) : num[k]);
        if (weight) weight[idx] = nan ? NAN : den;
    }
    // counts: one integer atomic per wavefront and count
    const unsigned long long hit = __ballot(active && !nan && den != 0.0);
    const unsigned long long nonfin = __ballot(active && !fin);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (hit && !bad) atomicAdd(reinterpret_cast<unsigned long long *>(&info->counts[0]), (unsigned long long)__popcll(hit));
        if (nonfin) atomicAdd(reinterpret_cast<unsigned long long *>(&info->counts[1]), (unsigned long long)__popcll(nonfin));
    }
}

struct WalkArgs {
    const double *px, *py, *pz;
    const uint32_t *pidx;
    int64_t m;
    Info *info;
    const double4 *rec;
    const double *wsa;
    const Ent *tab;
    uint64_t mask;
    double h_one;
    int normalise;
    double *out, *weight;
};

template <int K>
hipError_t launch_walk(bool per_h, hipStream_t st, const WalkArgs &a) {
    const dim3 grid(blocks(a.m, SB)), block(SB);
    if (per_h)
        sample_walk<K, true><<<grid, block, 0, st>>>(a.px, a.py, a.pz, a.pidx, a.m, a.info, a.rec, a.wsa, a.tab, a.mask, a.h_one,
                                                     a.normalise, a.out, a.weight);
    else
        sample_walk<K, false><<<grid, block, 0, st>>>(a.px, a.py, a.pz, a.pidx, a.m, a.info, a.rec, a.wsa, a.tab, a.mask, a.h_one,
                                                      a.normalise, a.out, a.weight);
    return hipGetLastError();
}

}  // namespace

int sample_build(sph_ctx *c, const SampleSources &src, size_t extra_bytes, SampleView *view, char **extra, char **sort_tmp_out) {
    hipStream_t st = c->stream;
    const int64_t n = c->n;
    const int64_t ns = c->cap > 0 ? c->n_slots : 0;
    const bool held = ns > 0 && n > 0;
    const bool per_h = src.per_h, host = src.host;
    const int nf = src.nf;
    // (SampleSwitches: A/B switches for the measurements of DESIGN.md section 13; the results do not depend on them beyond the level order)
    const int g0 = SampleSwitches().level_width;                           // 2^g0 quarter octaves per level
    const int64_t nn = std::max<int64_t>(n, 1);
    const int nb = (int)std::min<int64_t>((std::max<int64_t>(ns, 1) + SB - 1) / SB, BOX_BLOCKS);
    int64_t tl = 1;
    while (tl < 2 * nn) tl <<= 1;                                // hash table: load <= 1/2
    size_t sort_bytes = 0;
    SPH_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, (size_t)nn, 0u, 64u, st));
    const size_t n_val = host && src.values ? (size_t)nf * (size_t)nn : 0;
    uint64_t *keys, *keys_alt;
    uint32_t *vals, *vals_alt, *hist_buf;
    char *sort_tmp, *extra_buf;
    double4 *rec;
    Ent *tab;
    Info *info;
    double *wsa, *box_part, *h_values;
    auto layout = [&](Carve cv) {
        keys = cv.take<uint64_t>(nn);
        keys_alt = cv.take<uint64_t>(nn);
        vals = cv.take<uint32_t>(nn);
        vals_alt = cv.take<uint32_t>(nn);
        sort_tmp = cv.take<char>(std::max(sort_bytes, src.tmp_bytes));
        rec = cv.take<double4>(nn);
        wsa = cv.take<double>((size_t)(nf + 1) * (size_t)nn);
        tab = cv.take<Ent>(tl);
        box_part = cv.take<double>(NBP * (size_t)nb);
        hist_buf = cv.take<uint32_t>(per_h ? HBINS : 0);
        info = cv.take<Info>(1);
        h_values = cv.take<double>(n_val);                       // the host form's device copy
        extra_buf = cv.take<char>(extra_bytes);
        return cv.bytes;
    };
    char *buf = nullptr;
    SPH_TRY(analysis_scratch(c, layout(Carve{}), &buf));
    layout(Carve{buf});
    uint32_t *hist = per_h ? hist_buf : nullptr;
    const double *d_values = host && src.values ? h_values : src.values;

    Sel s{};
    for (int a = 0; a < 3; a++) { s.clip_lo[a] = src.clip_lo[a]; s.clip_hi[a] = src.clip_hi[a]; }
    s.h_one = src.h_one;
    s.hf = per_h ? c->f[SPH_F_H] : nullptr;
    s.n_owned = c->n_owned;
    Vals vf{};
    for (int k = 0; k < nf; k++) {
        const bool by_id = src.fields[k] == SPH_SAMPLE_VALUES;
        vf.by_id[k] = by_id ? 1 : 0;
        vf.ptr[k] = by_id ? d_values + (size_t)k * (size_t)n : c->f[src.fields[k]];
        if (by_id && host && n > 0)
            SPH_HIP(hipMemcpyAsync(const_cast<double *>(vf.ptr[k]), src.values + (size_t)k * (size_t)n, (size_t)n * sizeof(double),
                                   hipMemcpyHostToDevice, st));
    }
    const uint64_t mask = (uint64_t)(tl - 1);
    if (held) {
        const double *x = c->f[SPH_F_X], *y = c->f[SPH_F_Y], *z = c->f[SPH_F_Z];
        // selection, box, levels
        if (hist) SPH_HIP(hipMemsetAsync(hist, 0, sizeof(uint32_t) * (size_t)HBINS, st));
        sample_select<<<dim3((unsigned)nb), dim3(SB), 0, st>>>(x, y, z, c->orig, ns, s, box_part, hist);
        sample_levels<<<dim3(1), dim3(WAVE), 0, st>>>(box_part, nb, hist, src.h_one, g0, info);
        SPH_HIP(hipGetLastError());
        // (level, cell) keys by original id, sort, records, hash table over the occupied cells
        SPH_HIP(hipMemsetAsync(keys, 0xff, sizeof(uint64_t) * (size_t)n, st));
        SPH_HIP(hipMemsetAsync(vals, 0, sizeof(uint32_t) * (size_t)n, st));
        sample_keys<<<dim3(blocks(ns, SB)), dim3(SB), 0, st>>>(x, y, z, c->orig, ns, s, info, keys, vals);
        size_t tmp = sort_bytes;
        SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, keys, keys_alt, vals, vals_alt, (size_t)n, 0u, 64u, st));
        SPH_HIP(hipMemsetAsync(tab, 0xff, sizeof(Ent) * (size_t)tl, st));
        sample_records<<<dim3(blocks(n, SB)), dim3(SB), 0, st>>>(x, y, z, c->f[SPH_F_M], src.volume ? c->f[SPH_F_RHO] : nullptr,
                                                                 c->orig, s, vf, nf, keys_alt, vals_alt, info, n, rec, wsa, tab, mask);
        sample_tails<<<dim3(blocks(n, SB)), dim3(SB), 0, st>>>(keys_alt, info, n, tab, mask);
    } else {
        sample_no_sources<<<dim3(1), dim3(WAVE), 0, st>>>(info);
    }
    SPH_HIP(hipGetLastError());
    *view = SampleView{info, rec, wsa, tab, mask};
    *extra = extra_buf;
    *sort_tmp_out = sort_tmp;
    return SPH_OK;
}

int sample_run(sph_ctx *c, const sph_sample_desc *d, int64_t n_points, const double *px, const double *py, const double *pz,
               const double *values, double *out, int64_t n_out, double *weight, int64_t *counts, bool host) {
    const char *who = "sph_sample";
    if (!d) return arg_error(c, who, "null descriptor");
    if (d->reserved != 0) return arg_error(c, who, "reserved must be 0");
    if (d->flags & ~SPH_SAMPLE_NORMALISE) return arg_error(c, who, "unknown flags");
    if (n_points < 0 || n_points > 0x7fffffffLL) return arg_error(c, who, "n_points must be 0 .. 2^31 - 1");
    if (n_points > 0 && (!px || !py || !pz)) return arg_error(c, who, "null point arrays");
    const int nf = d->n_fields;
    if (nf < 0 || nf > SPH_SAMPLE_MAX_FIELDS) return arg_error(c, who, "n_fields must be 0 .. SPH_SAMPLE_MAX_FIELDS");
    bool any_values = false;
    for (int k = 0; k < nf; k++) {
        if (d->fields[k] != SPH_SAMPLE_VALUES && (d->fields[k] < 0 || d->fields[k] >= SPH_F_COUNT))
            return arg_error(c, who, "field id out of range");
        any_values = any_values || d->fields[k] == SPH_SAMPLE_VALUES;
    }
    if (any_values != (values != nullptr)) return arg_error(c, who, "values must be given with SPH_SAMPLE_VALUES and only then");
    if (n_out != (int64_t)nf * n_points) return arg_error(c, who, "n_out != n_fields n_points");
    if (!out && n_out > 0) return arg_error(c, who, "null output");
    if (nf == 0 && !weight) return arg_error(c, who, "n_fields == 0 needs the weight output");
    if (d->weight != SPH_RENDER_WEIGHT_MASS && d->weight != SPH_RENDER_WEIGHT_VOLUME) return arg_error(c, who, "unknown weight");
    if (std::isnan(d->h) || d->h < 0.0) return arg_error(c, who, "h must be >= 0");
    for (int a = 0; a < 3; a++)
        if (std::isnan(d->clip_lo[a]) || std::isnan(d->clip_hi[a])) return arg_error(c, who, "the clip box has a NaN");
    const bool volume = d->weight == SPH_RENDER_WEIGHT_VOLUME;
    bool stale = volume && !field_ready(*c, c->variable, SPH_F_RHO);
    for (int k = 0; k < nf; k++) stale = stale || (d->fields[k] >= 0 && !field_ready(*c, c->variable, d->fields[k]));
    if (stale) {
        c->err = "sph_sample: a field or rho is stale (sph_download_field would refuse it)";
        return SPH_ERR_STATE;
    }
    const bool per_h = !(d->h > 0.0) && c->variable;
    const double h_one = d->h > 0.0 ? d->h : (c->variable ? 0.0 : c->p.h);
    if (!per_h && !(h_one > 0.0)) {
        c->err = "sph_sample: params.h <= 0 on a fixed-h context (give desc.h > 0)";
        return SPH_ERR_STATE;
    }
    if (n_points == 0) {
        if (host) {
            if (counts) { counts[0] = 0; counts[1] = 0; }
        } else if (counts) {
            SPH_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), c->stream));
        }
        return SPH_OK;
    }

    hipStream_t st = c->stream;
    const int64_t m = n_points;
    const bool sort_points = SampleSwitches().point_sort;
    size_t psort_bytes = 0;
    if (sort_points)
        SPH_HIP(rocprim::radix_sort_pairs(nullptr, psort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                          (uint32_t *)nullptr, (size_t)m, 0u, (unsigned)(3 * LEVEL_AXIS_BITS + 1), st));
    const size_t mp = sort_points ? (size_t)m : 0;
    uint64_t *pkeys, *pkeys_alt;
    uint32_t *pvals, *pvals_alt;
    double *h_pts, *h_out, *h_weight;
    auto layout = [&](Carve cv) {
        pkeys = cv.take<uint64_t>(mp);
        pkeys_alt = cv.take<uint64_t>(mp);
        pvals = cv.take<uint32_t>(mp);
        pvals_alt = cv.take<uint32_t>(mp);
        h_pts = cv.take<double>(host ? 3 * (size_t)m : 0);       // the host form's device copies
        h_out = cv.take<double>(host ? n_out : 0);
        h_weight = cv.take<double>(host && weight ? m : 0);
        return cv.bytes;
    };
    const SampleSources src{d->clip_lo, d->clip_hi, h_one, per_h, volume, host, nf, d->fields, values, psort_bytes};
    SampleView v{};
    char *extra = nullptr, *sort_tmp = nullptr;
    SPH_TRY(sample_build(c, src, layout(Carve{}), &v, &extra, &sort_tmp));
    layout(Carve{extra});
    const double *d_px = px, *d_py = py, *d_pz = pz;
    if (host) {
        SPH_TRY(analysis_pinned(c));
        SPH_HIP(hipMemcpyAsync(h_pts, px, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        SPH_HIP(hipMemcpyAsync(h_pts + m, py, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        SPH_HIP(hipMemcpyAsync(h_pts + 2 * m, pz, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
        d_px = h_pts; d_py = h_pts + m; d_pz = h_pts + 2 * m;
    }
    double *d_out = host ? h_out : out;
    double *d_weight = host ? (weight ? h_weight : nullptr) : weight;
    Info *info = v.info;
    // the points in the order of their cells
    if (sort_points) {
        sample_point_keys<<<dim3(blocks(m, SB)), dim3(SB), 0, st>>>(d_px, d_py, d_pz, m, info, pkeys, pvals);
        SPH_HIP(hipGetLastError());
        size_t tmp = psort_bytes;
        SPH_HIP(rocprim::radix_sort_pairs(sort_tmp, tmp, pkeys, pkeys_alt, pvals, pvals_alt, (size_t)m, 0u,
                                          (unsigned)(3 * LEVEL_AXIS_BITS + 1), st));
    }
    WalkArgs wa{d_px, d_py, d_pz, sort_points ? pvals_alt : nullptr, m, info, v.rec, v.wsa, v.tab, v.mask, h_one,
                (d->flags & SPH_SAMPLE_NORMALISE) ? 1 : 0, d_out, d_weight};
    hipError_t e = hipSuccess;
    switch (nf) {
        case 0: e = launch_walk<0>(per_h, st, wa); break;
        case 1: e = launch_walk<1>(per_h, st, wa); break;
        case 2: e = launch_walk<2>(per_h, st, wa); break;
        case 3: e = launch_walk<3>(per_h, st, wa); break;
        default: e = launch_walk<4>(per_h, st, wa); break;
    }
    SPH_HIP(e);
    if (!host) {
        if (counts) SPH_HIP(hipMemcpyAsync(counts, info->counts, 2 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        return SPH_OK;
    }
    // host form: the counts, the rows and the weight in one read-back
    SPH_HIP(hipMemcpyAsync(c->rnd_pinned, info->counts, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (n_out > 0) SPH_HIP(hipMemcpyAsync(out, d_out, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    if (weight) SPH_HIP(hipMemcpyAsync(weight, d_weight, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
    SPH_HIP(hipStreamSynchronize(st));
    int64_t cnt[2] = {0, 0};
    std::memcpy(cnt, c->rnd_pinned, sizeof(cnt));
    if (cnt[0] < 0) {
        c->err = "sph_sample: a selected particle has h <= 0 or a non-finite h";
        return SPH_ERR_STATE;
    }
    if (counts) { counts[0] = cnt[0]; counts[1] = cnt[1]; }
    return SPH_OK;
}

}  // namespace sph
