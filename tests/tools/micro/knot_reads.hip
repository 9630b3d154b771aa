// Microbenchmark: how the two knots tab[k], tab[k + 1] of the kernel table are best fetched from LDS in the pair loop of the
// whole-tile kernels (density_wt, forces_q; pair_common.hpp table_knots_at) --
//   (a) one ds_read2_b64 offset1:1     (what the backend makes of two plain loads)
//   (b) two ds_read_b64                (volatile loads: the backend keeps them apart)
//   (c) one aligned ds_read_b128 from a doubled table of overlapping pairs {tab[k], tab[k + 1]} -- 80 KB, which does not fit beside
//       the kernels' tiles: for reference only, it bounds what a single read could give (its tile here is 64 KB, not 100)
// with the LDS queue looking like the kernels': between two knot fetches a lane reads one random record of a 100-KB tile,
// mode "32": two ds_read_b128 of a 32-byte record (density_wt), mode "96": the six 16-byte units of a record at 96-byte stride
// (forces_q).  One 1024-thread workgroup per CU, a 40-KB table (nq = 5118: 5120 doubles).
// Knot indices as the pair loop draws them: k = (int)(min(q, 2) nq / 2) with q^2 uniform on [0, 4] (the neighbour distances of a
// uniform disc: the number of partners within r grows as r^2), drawn per lane and visit on the host with a fixed seed; record slots
// uniform over the tile.  Both come packed in one 4-byte word per lane and visit, read coalesced like the kernels' list rows; every
// workgroup reads the same 1-MB stream (it stays in L2).
//   hipcc -O3 --offload-arch=gfx950 knot_reads.hip -o knot_reads && ./knot_reads
// Prints, per mode and variant, REP timings: ns per visit of a wave per CU (launch time / (VIS visits x 16 waves)) and the same in
// cycles at the clock rate the runtime reports.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(_e)); return 1; } } while (0)

constexpr int BS = 1024;
constexpr int VIS = 256;               // visits per lane and launch
constexpr int NQ = 5118;               // table: NQ + 2 = 5120 doubles = 40 KB
constexpr int TAB = NQ + 2;
constexpr int TILE_BYTES = 100 * 1024;
constexpr int TILE_BYTES_C = 64 * 1024;
constexpr int REP = 5;

// VAR: 0 = (a), 1 = (b), 2 = (c).  UNITS: 16-byte units read per record (2: 32-byte records, 6: 96-byte stride)
template <int VAR, int UNITS>
__global__ __launch_bounds__(BS) void knot_reads(const uint32_t *__restrict__ stream, int nslot, double *__restrict__ out) {
    extern __shared__ __align__(16) double lds[];
    constexpr int TABD = VAR == 2 ? 2 * TAB : TAB;
    double *tab = lds;
    double2 *tile = reinterpret_cast<double2 *>(lds + TABD);
    const int tile_units = nslot * UNITS;
    for (int k = threadIdx.x; k < TAB; k += BS) {
        const double v = 1.0 / (1.0 + k), v1 = 1.0 / (2.0 + k);
        if (VAR == 2) { tab[2 * k] = v; tab[2 * k + 1] = k + 1 < TAB ? v1 : 0.0; } else tab[k] = v;
    }
    for (int t = threadIdx.x; t < tile_units; t += BS) tile[t] = make_double2(1e-3 * (t % 977), 1.0);
    __syncthreads();
    double acc = 0.0;
    uint32_t w = stream[threadIdx.x];
    for (int v = 0; v < VIS; v++) {
        const uint32_t wn = stream[(size_t)min(v + 1, VIS - 1) * BS + threadIdx.x];
        const int k = (int)(w & 0xffffu), s = (int)(w >> 16);
        double t0, t1;
        if (VAR == 0) {
            t0 = tab[k]; t1 = tab[k + 1];
        } else if (VAR == 1) {
            typedef const volatile __attribute__((address_space(3))) double *LdsKnot;      // (a generic volatile pointer loads through flat_load)
            const LdsKnot p = (LdsKnot)(tab + k);
            t0 = p[0]; t1 = p[1];
        } else {
            const double2 t = reinterpret_cast<const double2 *>(tab)[k];
            t0 = t.x; t1 = t.y;
        }
        const double2 *r = tile + s * UNITS;
        double rs = 0.0;
#pragma unroll
        for (int u = 0; u < UNITS; u++) { const double2 q = r[u]; rs = fma(q.x, q.y, rs); }
        acc = fma(t0, rs, acc) + t1;
        w = wn;
    }
    out[(size_t)blockIdx.x * BS + threadIdx.x] = acc;
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int ncu = prop.multiProcessorCount;
    const double ghz = prop.clockRate * 1e-6;
    printf("%s: %d CUs, %.2f GHz; %d visits per lane, %d-thread workgroup per CU, table %d doubles\n", prop.name, ncu, ghz, VIS, BS, TAB);
    uint32_t *d_stream; double *d_out;
    CK(hipMalloc(&d_stream, (size_t)VIS * BS * 4));
    CK(hipMalloc(&d_out, (size_t)ncu * BS * 8));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    double ref = 0.0;
    auto run = [&](const char *name, auto kern, int units, int tile_bytes, size_t tab_bytes, bool check) -> int {
        const int nslot = tile_bytes / (16 * units);            // every slot, and so every read, lies inside the tile
        std::vector<uint32_t> st((size_t)VIS * BS);
        srand(7);
        for (auto &x : st) {
            const double q = std::sqrt(4.0 * (rand() / (RAND_MAX + 1.0)));
            const int k = (int)(std::fmin(q, 2.0) * (0.5 * NQ));    // <= NQ: k + 1 <= NQ + 1 = TAB - 1
            x = (uint32_t)k | ((uint32_t)(rand() % nslot) << 16);
        }
        CK(hipMemcpy(d_stream, st.data(), st.size() * 4, hipMemcpyHostToDevice));
        const size_t lds = tab_bytes + (size_t)tile_bytes;
        CK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        for (int w = 0; w < 3; w++) kern<<<ncu, BS, lds>>>(d_stream, nslot, d_out);
        CK(hipGetLastError());
        printf("%-52s", name);
        for (int rep = 0; rep < REP; rep++) {
            CK(hipEventRecord(e0));
            for (int w = 0; w < 10; w++) kern<<<ncu, BS, lds>>>(d_stream, nslot, d_out);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            const double ns = ms * 1e6 / 10 / ((double)VIS * (BS / 64));
            printf(" %6.2f ns (%5.1f cyc)", ns, ns * ghz);
        }
        double sum = 0.0;
        std::vector<double> o(BS);
        CK(hipMemcpy(o.data(), d_out, BS * 8, hipMemcpyDeviceToHost));
        for (double x : o) sum += x;
        if (check) printf("  %s", sum == ref ? "same sums" : "SUMS DIFFER"); else ref = sum;
        printf("\n");
        return 0;
    };
    const size_t tb = (size_t)TAB * 8;
    if (run("32-byte records  (a) ds_read2_b64 offset1:1", knot_reads<0, 2>, 2, TILE_BYTES, tb, false)) return 1;
    if (run("32-byte records  (b) two ds_read_b64", knot_reads<1, 2>, 2, TILE_BYTES, tb, true)) return 1;
    if (run("32-byte records  (c) ds_read_b128, doubled table", knot_reads<2, 2>, 2, TILE_BYTES_C, 2 * tb, false)) return 1;
    if (run("96-byte stride   (a) ds_read2_b64 offset1:1", knot_reads<0, 6>, 6, TILE_BYTES, tb, false)) return 1;
    if (run("96-byte stride   (b) two ds_read_b64", knot_reads<1, 6>, 6, TILE_BYTES, tb, true)) return 1;
    if (run("96-byte stride   (c) ds_read_b128, doubled table", knot_reads<2, 6>, 6, TILE_BYTES_C, 2 * tb, false)) return 1;
    return 0;
}
