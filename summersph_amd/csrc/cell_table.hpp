// cell_table.hpp -- the hashed table over the occupied cells of a sorted particle sequence, as sph_groups, sph_gradients and
// sph_sample build it (groups.hip, gradients.hip, sample.hip; not the step loop's hashed grid of grid.hip, which is a different table).
//
// A cell is the 63-bit key cx << 42 | cy << 21 | cz of its integer coordinates in a box {lo, 1 / edge}, 21 bits per axis.
// The particles are radix-sorted by key; the table maps every occupied key to the sorted positions [start, end) of its
// cell.  Open addressing with linear probing from hash_mix(key) & mask, the empty marker is key = ~0 (the caller fills the
// table with 0xff bytes first) and the table has at least twice as many entries as there can be cells: load <= 1/2.
// start is written by the cell's first sorted position (cell_enter), end by its last (cell_close, in a later launch).
// Which entry a key lands in depends on the order the lanes run in; what a lookup returns does not, and that keeps both
// modules' results bitwise the same over grids and slot orders.
#pragma once
#include "sph_internal.hpp"

namespace sph {

constexpr int AXIS_BITS = 21;
constexpr uint64_t AXIS_MASK = ((uint64_t)1 << AXIS_BITS) - 1;
constexpr double AXIS_CELLS = (double)((1 << AXIS_BITS) - 8);     // cells per axis the edge is enlarged to stay under

struct Ent { uint64_t key; int32_t start, end; };    // hash table entry; empty: key = ~0

__device__ __forceinline__ uint64_t cell_axis(double p, double lo, double inv_e) {
    // fmax drops a NaN (an overflowing product) to 0; the clamp keeps every key inside its 21 bits
    return (uint64_t)fmin(fmax(floor((p - lo) * inv_e), 0.0), (double)AXIS_MASK);
}

__device__ __forceinline__ uint64_t cell_key(double px, double py, double pz, const double *lo, double inv_e) {
    return (cell_axis(px, lo[0], inv_e) << (2 * AXIS_BITS)) | (cell_axis(py, lo[1], inv_e) << AXIS_BITS) |
           cell_axis(pz, lo[2], inv_e);
}

// Several cell grids in one table (sample.hip: one grid per level of smoothing lengths over the same box): the key
// level << 57 | cx << 38 | cy << 19 | cz with 6 bits of level and 19 bits per axis.  Key order is (level, cell).
constexpr int LEVEL_AXIS_BITS = 19;
constexpr int LEVEL_BITS = 6;
constexpr int MAX_LEVELS = 1 << LEVEL_BITS;
constexpr uint64_t LEVEL_AXIS_MASK = ((uint64_t)1 << LEVEL_AXIS_BITS) - 1;
constexpr double LEVEL_AXIS_CELLS = (double)((1 << LEVEL_AXIS_BITS) - 8);     // cells per axis a level's edge is enlarged to stay under

__device__ __forceinline__ uint64_t level_key(uint64_t level, uint64_t cx, uint64_t cy, uint64_t cz) {
    return (level << (3 * LEVEL_AXIS_BITS)) | (cx << (2 * LEVEL_AXIS_BITS)) | (cy << LEVEL_AXIS_BITS) | cz;
}

// the cell of a particle inside the box along one axis, clamped to [0, cmax] (cmax < 2^19)
__device__ __forceinline__ uint64_t level_cell_axis(double p, double lo, double inv_e, int32_t cmax) {
    return (uint64_t)fmin(fmax(floor((p - lo) * inv_e), 0.0), (double)cmax);
}

// the entry of key, or -1 when the table does not hold it
__device__ __forceinline__ int64_t hash_slot(const Ent *__restrict__ tab, uint64_t mask, uint64_t key) {
    for (uint64_t t = hash_mix(key) & mask;; t = (t + 1) & mask) {
        const uint64_t k = tab[t].key;
        if (k == key) return (int64_t)t;
        if (k == ~0ull) return -1;
    }
}

// sorted position p enters its cell into the table if it is the cell's first
__device__ __forceinline__ void cell_enter(const uint64_t *__restrict__ skey, int64_t p, Ent *__restrict__ tab, uint64_t mask) {
    const uint64_t key = skey[p];
    if (p > 0 && skey[p - 1] == key) return;
    for (uint64_t t = hash_mix(key) & mask;; t = (t + 1) & mask) {
        const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(&tab[t].key), ~0ull,
                                                  (unsigned long long)key);
        if (prev == ~0ull) { tab[t].start = (int32_t)p; return; }     // every key is inserted once: by its first position
    }
}

// sorted position p of n_live (the launch covers n >= n_live positions) closes its cell if it is the cell's last
__device__ __forceinline__ void cell_close(const uint64_t *__restrict__ skey, int64_t p, int64_t n, int64_t n_live,
                                           Ent *__restrict__ tab, uint64_t mask) {
    if (p >= n || p >= n_live) return;
    const uint64_t key = skey[p];
    if (p + 1 < n_live && skey[p + 1] == key) return;
    const int64_t t = hash_slot(tab, mask, key);           // put there by the cell's first position
    if (t >= 0) tab[t].end = (int32_t)(p + 1);
}

}  // namespace sph
