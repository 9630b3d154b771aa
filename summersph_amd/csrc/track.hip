// track.hip -- trajectories and fates of chosen particles (include/summersph.h, sph_track): a device-resident log that
// receives one row per recorded step, holding the state of K particles named by their caller-order ids at sph_track_begin.
// A name survives every renumbering: the accretion pack (accrete.hip, pack_survivors) calls track_repack, which moves the
// ids with pack()'s scan and writes the fate of whoever left.  The host keeps the row index, the step number and the dropped
// count; the live count stays on the device.  A recorded step waits for nothing and reads nothing back.
//
// Only reads the context: the state, the grid, the list, the statistics, dt and every validity flag stay as they are, and
// with no tracker begun the step and the pack enqueue exactly what they enqueued before.
//
// Membership and rank.  bitmap: one bit per caller id (set: tracked and alive).  prefix[w]: set bits below word w.
// rank(id) = prefix[id / 64] + popcount(word & bits below id) is the particle's index among the live tracked ones in id
// order, and tag[rank] the tracked index k.  One launch per recorded row:
//   track_row      grid-stride over the sorted slots: orig[slot] read in order, one bit test; a hit (rare: K << n) writes
//                  the ten values of its slot into column k of the row.  Thread 0 writes the row's head.
// and, at begin and after a pack that removed particles (never otherwise):
//   track_repack   one thread per tracked k: a survivor's id becomes pos[id], a removed particle gets its fate
//   track_bits     the bitmap (cleared before) from the live ids, by vector atomics
//   track_prefix   one block: the exclusive scan of the words' popcounts
//   track_tags     tag[rank(id_k)] = k
#include <new>

#include "sph_internal.hpp"

namespace sph {

namespace {

constexpr int TB = 256;                    // block of every kernel but the scan
constexpr int T_BLOCKS = 2048;             // blocks of track_row at most (grid-stride beyond)
constexpr int PB = 1024;                   // the scan's one block
constexpr int NCOL = SPH_TRACK_NCOL, NHEAD = SPH_TRACK_NHEAD;

struct Cols {
    const double *f[NCOL];                 // x y z vx vy vz u rho h alpha in sorted order; null: rho is not current / h is fixed
    double h_fixed;
};

// word: the bitmap word of id
__device__ __forceinline__ int rank_of(const int32_t *__restrict__ prefix, int32_t id, unsigned long long word) {
    return prefix[id >> 6] + __popcll(word & ((1ull << (id & 63)) - 1ull));
}

__global__ __launch_bounds__(TB) void track_row(Cols c, const int32_t *__restrict__ orig, int64_t n_slots, int64_t n_bits,
                                                const unsigned long long *__restrict__ bitmap,
                                                const int32_t *__restrict__ prefix, const int32_t *__restrict__ tag, int64_t K,
                                                const double *__restrict__ d_dt, double step, double n_gas,
                                                const int32_t *__restrict__ live, double *__restrict__ head,
                                                double *__restrict__ body) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        head[0] = step;
        head[1] = d_dt[1];
        head[2] = n_gas;
        head[3] = (double)*live;
    }
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * TB) {
        const int32_t id = orig[i];
        if (id < 0 || id >= n_bits) continue;
        const unsigned long long word = bitmap[id >> 6];
        if (!(word >> (id & 63) & 1ull)) continue;
        const int64_t k = tag[rank_of(prefix, id, word)];
#pragma unroll
        for (int q = 0; q < NCOL; q++) {
            double v;
            if (c.f[q]) v = c.f[q][i];
            else v = q == 8 ? c.h_fixed : (double)NAN;
            body[(int64_t)q * K + k] = v;
        }
    }
}

// fates[4 k ..]: {fate, step, sink, current id}.  keep / pos by caller id, accmask by sorted slot (accrete.hip)
__global__ __launch_bounds__(TB) void track_repack(int64_t K, int32_t *__restrict__ fates, const int32_t *__restrict__ keep,
                                                   const int32_t *__restrict__ pos, const int32_t *__restrict__ inv,
                                                   const unsigned long long *__restrict__ accmask, int32_t step,
                                                   int32_t *__restrict__ live) {
    const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= K) return;
    const int32_t id = fates[4 * k + 3];
    if (id < 0) return;
    if (keep[id]) { fates[4 * k + 3] = pos[id]; return; }
    const unsigned long long mask = accmask[inv[id]];
    fates[4 * k + 0] = mask ? 1 : 2;
    fates[4 * k + 1] = step;
    fates[4 * k + 2] = mask ? __ffsll((long long)mask) - 1 : -1;     // the first sink whose sums took it (acc_sums_partial)
    fates[4 * k + 3] = -1;
    atomicSub(live, 1);
}

__global__ __launch_bounds__(TB) void track_bits(int64_t K, const int32_t *__restrict__ fates,
                                                 unsigned long long *__restrict__ bitmap) {
    const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= K) return;
    const int32_t id = fates[4 * k + 3];
    if (id >= 0) atomicOr(&bitmap[id >> 6], 1ull << (id & 63));
}

// one block: thread t owns a contiguous run of words
__global__ __launch_bounds__(PB) void track_prefix(const unsigned long long *__restrict__ bitmap, int64_t n_words,
                                                   int32_t *__restrict__ prefix) {
    __shared__ int32_t s[PB];
    const int t = threadIdx.x;
    const int64_t per = (n_words + PB - 1) / PB;
    const int64_t lo = t * per < n_words ? t * per : n_words, hi = lo + per < n_words ? lo + per : n_words;
    int32_t sum = 0;
    for (int64_t w = lo; w < hi; w++) sum += __popcll(bitmap[w]);
    s[t] = sum;
    __syncthreads();
    for (int o = 1; o < PB; o <<= 1) {
        const int32_t v = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int32_t base = s[t] - sum;
    for (int64_t w = lo; w < hi; w++) { prefix[w] = base; base += __popcll(bitmap[w]); }
}

__global__ __launch_bounds__(TB) void track_tags(int64_t K, const int32_t *__restrict__ fates,
                                                 const unsigned long long *__restrict__ bitmap,
                                                 const int32_t *__restrict__ prefix, int32_t *__restrict__ tag) {
    const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= K) return;
    const int32_t id = fates[4 * k + 3];
    if (id >= 0) tag[rank_of(prefix, id, bitmap[id >> 6])] = (int32_t)k;
}

}  // namespace

struct Track {
    sph_track_desc d{};
    int64_t K = 0, n_bits = 0, n_words = 0;
    int64_t rows = 0, dropped = 0, steps = 0;
    bool closed = false;
    double *head = nullptr, *body = nullptr;             // capacity x NHEAD, capacity x NCOL x K
    unsigned long long *bitmap = nullptr;
    int32_t *prefix = nullptr, *tag = nullptr, *fates = nullptr, *live = nullptr;
};

void track_free(sph_ctx *c) {
    Track *t = c->track;
    if (!t) return;
    ctx_free(c, t->head); ctx_free(c, t->body); ctx_free(c, t->bitmap); ctx_free(c, t->prefix); ctx_free(c, t->tag);
    ctx_free(c, t->fates); ctx_free(c, t->live);
    delete t;
    c->track = nullptr;
}

void track_close(sph_ctx *c) { if (c->track) c->track->closed = true; }

// bitmap, prefix and tags from the current ids
static int track_rebuild(sph_ctx *c) {
    Track *t = c->track;
    hipStream_t st = c->stream;
    const unsigned kb = blocks(t->K, TB);
    SPH_HIP(hipMemsetAsync(t->bitmap, 0, (size_t)t->n_words * sizeof(unsigned long long), st));
    track_bits<<<dim3(kb), dim3(TB), 0, st>>>(t->K, t->fates, t->bitmap);
    track_prefix<<<dim3(1), dim3(PB), 0, st>>>(t->bitmap, t->n_words, t->prefix);
    track_tags<<<dim3(kb), dim3(TB), 0, st>>>(t->K, t->fates, t->bitmap, t->prefix, t->tag);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

int track_begin(sph_ctx *c, const sph_track_desc *d, int64_t n_ids, const int64_t *ids, bool host) {
    const char *who = host ? "sph_track_begin" : "sph_track_begin_dev";
    if (!d) return arg_error(c, who, "null descriptor");
    if (d->capacity < 1) return arg_error(c, who, "capacity must be >= 1");
    if (d->every < 1) return arg_error(c, who, "every must be >= 1");
    if (d->flags != 0) return arg_error(c, who, "flags must be 0");
    if (n_ids < 1) return arg_error(c, who, "n_ids must be >= 1");
    if (!ids) return arg_error(c, who, "null ids");
    if (c->nranks > 1 || c->n_owned != c->n) { c->err = std::string(who) + ": one rank and no ghost particles"; return SPH_ERR_STATE; }
    if (n_ids > c->n) return arg_error(c, who, "more ids than particles: an id is outside [0, n) or given twice");
    std::vector<int64_t> from_dev;
    if (!host) {                                         // the ids are checked on the host in both forms: begin may wait
        from_dev.resize((size_t)n_ids);
        SPH_HIP(hipMemcpyAsync(from_dev.data(), ids, (size_t)n_ids * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        SPH_HIP(hipStreamSynchronize(c->stream));
        ids = from_dev.data();
    }
    std::vector<int32_t> f((size_t)4 * n_ids);
    {
        std::vector<bool> seen((size_t)c->n, false);
        for (int64_t k = 0; k < n_ids; k++) {
            if (ids[k] < 0 || ids[k] >= c->n) return arg_error(c, who, "an id is outside [0, n)");
            if (seen[(size_t)ids[k]]) return arg_error(c, who, "an id is given twice");
            seen[(size_t)ids[k]] = true;
            f[4 * k + 0] = 0; f[4 * k + 1] = 0; f[4 * k + 2] = -1; f[4 * k + 3] = (int32_t)ids[k];
        }
    }
    const double body_doubles = (double)d->capacity * (double)NCOL * (double)n_ids;
    if (body_doubles > 1.0e15) { c->err = std::string(who) + ": the log does not fit"; return SPH_ERR_NOMEM; }
    track_free(c);
    Track *t = new (std::nothrow) Track();
    if (!t) { c->err = std::string(who) + ": out of host memory"; return SPH_ERR_NOMEM; }
    c->track = t;
    t->d = *d;
    t->K = n_ids;
    t->n_bits = c->n;                                    // ids only ever decrease (pack() renumbers by rank)
    t->n_words = (c->n + 63) / 64;
    const size_t body = (size_t)d->capacity * NCOL * (size_t)n_ids;
    int st = ctx_alloc(c, &t->head, (size_t)d->capacity * NHEAD, "track heads");
    if (st == SPH_OK) st = ctx_alloc(c, &t->body, body, "track log");
    if (st == SPH_OK) st = ctx_alloc(c, &t->bitmap, (size_t)t->n_words, "track bitmap");
    if (st == SPH_OK) st = ctx_alloc(c, &t->prefix, (size_t)t->n_words, "track prefix");
    if (st == SPH_OK) st = ctx_alloc(c, &t->tag, (size_t)n_ids, "track tags");
    if (st == SPH_OK) st = ctx_alloc(c, &t->fates, (size_t)4 * n_ids, "track fates");
    if (st == SPH_OK) st = ctx_alloc(c, &t->live, 1, "track live count");
    if (st != SPH_OK) { track_free(c); return st; }
    const int32_t live = (int32_t)n_ids;
    hipError_t e = hipMemsetAsync(t->body, 0xFF, body * sizeof(double), c->stream);      // every byte 0xFF: a NaN
    if (e == hipSuccess) e = hipMemcpyAsync(t->fates, f.data(), f.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->live, &live, sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);        // f and live are this call's own
    if (e != hipSuccess) { track_free(c); SPH_HIP(e); }
    st = track_rebuild(c);
    if (st != SPH_OK) track_free(c);
    return st;
}

int track_end(sph_ctx *c) {
    if (!c->track) { c->err = "sph_track_end: no tracker begun"; return SPH_ERR_STATE; }
    track_free(c);
    return SPH_OK;
}

// appends the row of the state as it is now; a full log drops it and counts
static int track_append(sph_ctx *c) {
    Track *t = c->track;
    if (t->rows >= t->d.capacity) { t->dropped++; return SPH_OK; }
    const int64_t n_slots = c->cap > 0 ? c->n_slots : 0;
    Cols cols{};
    static const int src[NCOL] = {SPH_F_X, SPH_F_Y, SPH_F_Z, SPH_F_VX, SPH_F_VY, SPH_F_VZ, SPH_F_U, SPH_F_RHO, SPH_F_H, SPH_F_ALPHA};
    for (int q = 0; q < NCOL; q++) cols.f[q] = c->f[src[q]];
    if (!(n_slots > 0 && field_ready(*c, c->variable, SPH_F_RHO))) cols.f[7] = nullptr;
    if (!c->variable) cols.f[8] = nullptr;
    cols.h_fixed = c->p.h;
    const unsigned nb = std::min<unsigned>(blocks(n_slots, TB), T_BLOCKS);
    track_row<<<dim3(nb), dim3(TB), 0, c->stream>>>(cols, c->orig, n_slots, t->n_bits, t->bitmap, t->prefix, t->tag, t->K, c->d_dt,
                                                    (double)t->steps, (double)(n_slots > 0 ? c->n_owned : 0), t->live,
                                                    t->head + (size_t)t->rows * NHEAD, t->body + (size_t)t->rows * NCOL * (size_t)t->K);
    SPH_HIP(hipGetLastError());
    t->rows++;
    return SPH_OK;
}

int track_record(sph_ctx *c) {
    if (!c->track) { c->err = "sph_track_record: no tracker begun"; return SPH_ERR_STATE; }
    if (c->track->closed) { c->err = "sph_track_record: the tracker is closed (the particle set was replaced)"; return SPH_ERR_STATE; }
    return track_append(c);
}

int track_step(sph_ctx *c) {
    Track *t = c->track;
    if (!t || t->closed) return SPH_OK;
    t->steps++;
    if (t->steps % t->d.every != 0) return SPH_OK;
    return track_append(c);
}

int track_packed(sph_ctx *c, const int32_t *keep, const int32_t *pos, const unsigned long long *accmask) {
    Track *t = c->track;
    if (!t || t->closed) return SPH_OK;
    track_repack<<<dim3(blocks(t->K, TB)), dim3(TB), 0, c->stream>>>(t->K, t->fates, keep, pos, c->inv, accmask, (int32_t)t->steps,
                                                                    t->live);
    SPH_HIP(hipGetLastError());
    return track_rebuild(c);
}

int track_info(sph_ctx *c, int64_t *rows, int64_t *dropped, int64_t *steps, int64_t *n_tracked, int64_t *n_live, int32_t *closed) {
    const Track *t = c->track;
    if (!t) { c->err = "sph_track_info: no tracker begun"; return SPH_ERR_STATE; }
    if (rows) *rows = t->rows;
    if (dropped) *dropped = t->dropped;
    if (steps) *steps = t->steps;
    if (n_tracked) *n_tracked = t->K;
    if (closed) *closed = t->closed ? 1 : 0;
    if (n_live) {                                        // the one count that lives on the device
        int32_t live = 0;
        SPH_HIP(hipMemcpyAsync(&live, t->live, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        SPH_HIP(hipStreamSynchronize(c->stream));
        *n_live = live;
    }
    return SPH_OK;
}

int track_read(sph_ctx *c, int64_t first, int64_t count, double *head, double *body, bool host) {
    const char *who = host ? "sph_track_read" : "sph_track_read_dev";
    const Track *t = c->track;
    if (!t) { c->err = std::string(who) + ": no tracker begun"; return SPH_ERR_STATE; }
    if (first < 0 || count < 0 || first > t->rows || count > t->rows - first) return arg_error(c, who, "first / count outside [0, rows]");
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (count > 0 && head)
        SPH_HIP(hipMemcpyAsync(head, t->head + (size_t)first * NHEAD, (size_t)count * NHEAD * sizeof(double), kind, c->stream));
    if (count > 0 && body)
        SPH_HIP(hipMemcpyAsync(body, t->body + (size_t)first * NCOL * (size_t)t->K, (size_t)count * NCOL * (size_t)t->K * sizeof(double),
                               kind, c->stream));
    return SPH_OK;
}

int track_fates(sph_ctx *c, int32_t *fates, bool host) {
    const char *who = host ? "sph_track_fates" : "sph_track_fates_dev";
    const Track *t = c->track;
    if (!t) { c->err = std::string(who) + ": no tracker begun"; return SPH_ERR_STATE; }
    if (!fates) return arg_error(c, who, "null output");
    SPH_HIP(hipMemcpyAsync(fates, t->fates, (size_t)4 * (size_t)t->K * sizeof(int32_t), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           c->stream));
    return SPH_OK;
}

}  // namespace sph
