// gravity.hip -- Barnes-Hut gas self-gravity, reproducing the reference's tree walk.
//
// Replaces (citations: /root/reference/SUMMER_SPH.f90 "[F]"; "SUMMER_SPH - Variable.f90" "[V]")
//   create_tree / build_tree (masses, centres of mass)      [F]:795-816,149-246
//   particle_gravforces / particle_gravforce_one, theta 0.5 [F]:249-290  ([V]:285-311: softening table
//                                                           looked up with the particle's own h)
//
// The reference walks a pointer octree (bbox-midpoint root, edge = largest extent, strict '>' split, one
// particle per leaf) and accepts a node when edge / sqrt(|x - com|^2 + 0.001*2.5) < theta or when it is
// a leaf.  Here the same tree exists only implicitly:
//   * every particle's path down that octree is a 63-bit key (3 bits per level, varh.hip uses the same
//     keys for the leaf boxes); the keys are radix-sorted;
//   * a binary radix tree (Karras 2012) over the sorted keys gives all ranges of particles that share a
//     key prefix.  A binary node whose prefix length crosses a multiple of 3 IS an octree node (and, with
//     it, the whole chain of single-child octree nodes above it: same particles, same centre of mass,
//     larger edges); the others are partial groups that the reference never tests.  The walk therefore
//     tests acceptance only on the former, with the smallest edge of the chain (if any node of the chain
//     is accepted the contribution is the same), and opens the latter unconditionally;
//   * masses and centres of mass are summed bottom-up (pairwise, fixed order -> reproducible);
//   * the walk is stackless (rope pointers), one lane per target particle in cell-sorted order, so the
//     lanes of a wave walk nearly the same nodes.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pair_common.hpp"

namespace sph {

namespace {

constexpr int GB = 256;
constexpr int LEVELS = 21;
constexpr int END = 0x7fffffff;          // rope terminator

struct RootBox { double c[3]; double size; };

__global__ __launch_bounds__(GB) void grav_keys(RootBox rb, const double4 *__restrict__ drec, int64_t n,
                                                uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * GB + threadIdx.x;
    if (i >= n) return;
    const double4 p = drec[i];
    double cx = rb.c[0], cy = rb.c[1], cz = rb.c[2], size = rb.size;
    uint64_t key = 0;
    for (int l = 0; l < LEVELS; l++) {                        // [F]:208-217, 190-198
        const int bx = p.x > cx, by = p.y > cy, bz = p.z > cz;
        key = (key << 3) | (uint64_t)(bx | (by << 1) | (bz << 2));
        const double q = 0.25 * size;
        cx = cx + (bx ? q : -q); cy = cy + (by ? q : -q); cz = cz + (bz ? q : -q);
        size = size * 0.5;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

// common prefix length (in bits of the 64-bit word) of sorted keys i and j; ties are broken by the index
__device__ __forceinline__ int delta(const uint64_t *__restrict__ k, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const uint64_t x = k[i] ^ k[j];
    if (x == 0) return 64 + __clz(i ^ j);
    return __clzll((long long)x);
}

// node ids: internal i in [0, n-2] as i; leaf j as ~j (negative)
struct TreeArrays {
    int32_t *left, *right, *parent;     // internal nodes
    int32_t *leaf_parent;               // leaves
    int32_t *prefix;                    // internal: common prefix length (bits of the 64-bit word)
    int32_t *other;                     // internal: the far end j of the node's leaf range [min(i,j), max(i,j)]
    double4 *seg;                       // segment tree over the leaves in key order (levels 1.., see seg_stage)
    double4 *sum;                       // internal: sum m x, sum m y, sum m z, sum m  -> later com + mass
    double4 *leafA;                     // leaves in key order: x y z m
    int32_t *slot;                      // leaf -> cell-sorted slot
    int32_t *lvl;                       // internal: octree level of the node's smallest box, or -1 (partial group)
    int32_t *rope, *leaf_rope;          // next node after this subtree in depth-first order
    int4 *walkB;                        // internal: {first octree node / leaf below, rope, level, -} with partial
                                        // (non-octree) binary nodes skipped on both pointers
    int2 *leafB;                        // leaves: {rope (partial nodes skipped), cell-sorted slot}
};

__global__ __launch_bounds__(GB) void radix_tree(const uint64_t *__restrict__ k, int n, TreeArrays t) {
    const int i = blockIdx.x * GB + threadIdx.x;
    if (i >= n - 1) return;
    const int d = delta(k, n, i, i + 1) > delta(k, n, i, i - 1) ? 1 : -1;
    const int dmin = delta(k, n, i, i - d);
    int lmax = 2;
    while (delta(k, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int s = lmax >> 1; s >= 1; s >>= 1)
        if (delta(k, n, i, i + (l + s) * d) > dmin) l += s;
    const int j = i + l * d;
    const int dnode = delta(k, n, i, j);
    int s = 0;
    int tt = l;
    do {
        tt = (tt + 1) >> 1;
        if (delta(k, n, i, i + (s + tt) * d) > dnode) s += tt;
    } while (tt > 1);
    const int gamma = i + s * d + min(d, 0);
    const int lo = min(i, j), hi = max(i, j);
    const int L = lo == gamma ? ~gamma : gamma;
    const int Rr = hi == gamma + 1 ? ~(gamma + 1) : gamma + 1;
    t.left[i] = L; t.right[i] = Rr;
    t.prefix[i] = dnode;
    if (L < 0) t.leaf_parent[~L] = i; else t.parent[L] = i;
    if (Rr < 0) t.leaf_parent[~Rr] = i; else t.parent[Rr] = i;
    if (i == 0) t.parent[0] = -1;
    t.other[i] = j;
}

__global__ __launch_bounds__(GB) void leaf_data(const uint32_t *__restrict__ vals, const double4 *__restrict__ drec, int n,
                                                TreeArrays t) {
    const int j = blockIdx.x * GB + threadIdx.x;
    if (j >= n) return;
    const uint32_t s = vals[j];
    t.leafA[j] = drec[s];
    t.slot[j] = (int32_t)s;
}

// Node sums.  Every internal node of the radix tree covers a contiguous range of leaves (key order), so its mass
// and first moments are a range sum over the leaves.  A segment tree over the leaf array (level l entry k = sum of
// leaves [k 2^l, (k+1) 2^l), built in stages of SEG_LV levels per launch, LDS ping-pong) answers every range with
// 2 log2(length) entries, summed small to large on either side -- pairwise accuracy, a fixed order (reproducible),
// and no communication between workgroups (a bottom-up pass with arrival counters needs device-scope fences, which
// write back the XCD's L2 on this chip: 5.8 ms for 1e6 leaves, against 0.1 ms for this scheme).
constexpr int SEG_LV = 9;                       // levels per stage: a block reduces 512 entries
constexpr int SEG_MAX_LEVELS = 40;
struct SegLevels {
    int64_t off[SEG_MAX_LEVELS];                // off[l]: first entry of level l in seg[] (level 0 = the leaves, not stored)
    int64_t cnt[SEG_MAX_LEVELS];
    int levels;
};

__device__ __forceinline__ double4 leaf_moment(const double4 p) { return make_double4(p.w * p.x, p.w * p.y, p.w * p.z, p.w); }
__device__ __forceinline__ double4 add4(const double4 a, const double4 b) { return make_double4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// stage: from level L0 (the leaves if L0 == 0) up to level L0 + SEG_LV
__global__ __launch_bounds__(256) void seg_stage(SegLevels sl, int L0, const double4 *__restrict__ leafA, double4 *__restrict__ seg) {
    __shared__ double4 buf[2][512];
    const int64_t base = (int64_t)blockIdx.x * 512;
    const int64_t c0 = sl.cnt[L0];
    for (int e = threadIdx.x; e < 512; e += 256) {
        const int64_t k = base + e;
        double4 v = make_double4(0, 0, 0, 0);
        if (k < c0) v = L0 == 0 ? leaf_moment(leafA[k]) : seg[sl.off[L0] + k];
        buf[0][e] = v;
    }
    __syncthreads();
    int cur = 0;
    for (int l = 1; l <= SEG_LV && L0 + l < sl.levels; l++) {
        const int width = 512 >> l;
        const int64_t kb = base >> l;
        for (int e = threadIdx.x; e < width; e += 256) {
            const double4 v = add4(buf[cur][2 * e], buf[cur][2 * e + 1]);     // entries past the end are zero
            buf[cur ^ 1][e] = v;
            if (kb + e < sl.cnt[L0 + l]) seg[sl.off[L0 + l] + kb + e] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
}

__global__ __launch_bounds__(GB) void node_sums_seg(int n, SegLevels sl, TreeArrays t) {
    const int i = blockIdx.x * GB + threadIdx.x;
    if (i >= n - 1) return;
    const int j = t.other[i];
    int64_t l = min(i, j), r = (int64_t)max(i, j) + 1;
    double4 accl = make_double4(0, 0, 0, 0), accr = make_double4(0, 0, 0, 0);
    int lev = 0;
    while (l < r) {
        if (l & 1) { accl = add4(accl, lev == 0 ? leaf_moment(t.leafA[l]) : t.seg[sl.off[lev] + l]); l++; }
        if (r & 1) { r--; accr = add4(accr, lev == 0 ? leaf_moment(t.leafA[r]) : t.seg[sl.off[lev] + r]); }
        l >>= 1; r >>= 1; lev++;
    }
    t.sum[i] = add4(accl, accr);
}

// centre of mass, octree level, ropes
__global__ __launch_bounds__(GB) void node_finish(int n, TreeArrays t) {
    const int i = blockIdx.x * GB + threadIdx.x;
    if (i < n - 1) {
        const double4 s = t.sum[i];
        t.sum[i] = s.w > 0.0 ? make_double4(s.x / s.w, s.y / s.w, s.z / s.w, s.w) : make_double4(0, 0, 0, 0);   // [F]:173-177
        // key bits shared by the node's particles: prefix - 1 (the 64-bit word has a leading zero bit)
        const int bits = min(t.prefix[i] - 1, 3 * LEVELS);
        const int par = t.parent[i];
        const int pbits = par < 0 ? -1 : min(t.prefix[par] - 1, 3 * LEVELS);
        const int lv = bits / 3;
        t.lvl[i] = (3 * lv > pbits) ? lv : -1;
        // rope: next node after this subtree
        int x = i, r = END;
        while (x != 0) {
            const int p = t.parent[x];
            if (t.left[p] == x) { r = t.right[p]; break; }
            x = p;
        }
        t.rope[i] = r;
    }
    if (i < n) {
        int r = END;
        if (n >= 2) {
            int p = t.leaf_parent[i];
            if (t.left[p] == ~i) r = t.right[p];
            else {
                int x = p;
                while (x != 0) {
                    const int pp = t.parent[x];
                    if (t.left[pp] == x) { r = t.right[pp]; break; }
                    x = pp;
                }
            }
        }
        t.leaf_rope[i] = r;
    }
}

// The walk only ever TESTS octree nodes and leaves; partial binary nodes are opened unconditionally, so both
// pointers of the walk records jump over them: eff(x) = x if x is a leaf or an octree node, else eff(left(x)).
__device__ __forceinline__ int eff_node(const TreeArrays &t, int x) {
    while (x != END && x >= 0 && t.lvl[x] < 0) x = t.left[x];
    return x;
}

__global__ __launch_bounds__(GB) void node_walk_records(int n, TreeArrays t) {
    const int i = blockIdx.x * GB + threadIdx.x;
    if (i < n - 1) t.walkB[i] = make_int4(eff_node(t, t.left[i]), eff_node(t, t.rope[i]), t.lvl[i], 0);
    if (i < n) t.leafB[i] = make_int2(eff_node(t, t.leaf_rope[i]), t.slot[i]);
}

// the walk, [F]:264-290.  Writes a = 0 - sum (the forces kernels continue from there, [F]:824-827).
__global__ __launch_bounds__(GB) void grav_walk(int n, TreeArrays t, RootBox rb, const double4 *__restrict__ drec,
                                                const double *__restrict__ hvar, double hfix, double soft2, double theta, double G,
                                                const double *__restrict__ gt, int nq, double dq, double *__restrict__ ax,
                                                double *__restrict__ ay, double *__restrict__ az, const int32_t *__restrict__ orig,
                                                int32_t n_owned) {
    const int i = xcd_chunk(blockIdx.x, gridDim.x) * GB + threadIdx.x;
    if (i >= n) return;
    if (orig[i] >= n_owned) return;
    const double4 p = drec[i];
    const double hp = hvar ? hvar[i] : hfix;
    const double inv_hp = 1.0 / hp, inv_dq = 1.0 / dq, theta2 = theta * theta;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    // the root is an octree node by construction (level >= 0)
    int node = n >= 2 ? 0 : END;
    while (node != END) {
        double4 c;
        int next_open, next_skip;
        bool leaf;
        double size = 0.0;
        if (node < 0) {
            const int j = ~node;
            const int2 lb = t.leafB[j];
            next_skip = lb.x; next_open = lb.x;
            if (lb.y == i) { node = next_skip; continue; }           // own leaf: direction = 0, contributes nothing
            c = t.leafA[j];
            leaf = true;
        } else {
            const int4 wb = t.walkB[node];
            c = t.sum[node];
            leaf = false;
            size = ldexp(rb.size, -wb.z);
            next_open = wb.x; next_skip = wb.y;
        }
        const double d0 = p.x - c.x, d1 = p.y - c.y, d2c = p.z - c.z;  // [F]:274
        const double d2 = fma(d2c, d2c, fma(d1, d1, fma(d0, d0, soft2)));    // [F]:275
        // [F]:278: size/dist < theta  <=>  size^2 < theta^2 d2 (all positive): opened nodes need neither the
        // square root nor the division (the two forms can only disagree within an ulp of the threshold)
        if (leaf || size * size < theta2 * d2) {
            if (c.w > 0.0) {
                const double rs = fast_rsqrt(d2);
                double f = (G * c.w) * ((rs * rs) * rs);              // [F]:281: G M [W] / dist^3
                const double qi = (d2 * rs) * inv_hp;                  // dist / h
                if (qi <= 2.0) {                                       // [F]:129-146: W = 1 beyond the softening support
                    const double tq = qi * inv_dq;
                    const int k = min((int)tq, nq - 1);
                    const double a = tq - (double)k;
                    f *= (1.0 - a) * gt[k] + a * gt[k + 1];
                }
                a0 = fma(-f, d0, a0); a1 = fma(-f, d1, a1); a2 = fma(-f, d2c, a2);
            }
            node = next_skip;
        } else {
            node = next_open;
        }
    }
    ax[i] = a0; ay[i] = a1; az[i] = a2;
}

// One 64-byte record per node for the wave walk, leaves behind the internal nodes (unified index: internal i -> i,
// leaf j -> n - 1 + j): centre of mass + G x mass, the squared edge of the node's smallest box (-1 for a leaf: always
// accepted), both successors, and for leaves the cell-sorted slot (to recognise the target's own leaf).
struct alignas(64) WalkRec {
    double cx, cy, cz, gm;              // centre of mass, G m (first 32 bytes: what the contribution needs, one scalar load)
    double size2;
    int32_t next_open, next_skip;       // unified indices, END terminates
    int32_t slot, has_mass;             // has_mass: m > 0 (a wave-uniform test in the walk, not a vector compare)
    double pad;
};

__device__ __forceinline__ int unified(int node, int n) { return node == END ? END : (node < 0 ? n - 1 + ~node : node); }

__global__ __launch_bounds__(GB) void node_wave_records(int n, TreeArrays t, RootBox rb, double theta2, double G, WalkRec *__restrict__ rec,
                                                        int32_t *__restrict__ leaf_of) {
    const int i = blockIdx.x * GB + threadIdx.x;
    if (i < n - 1) {
        const int4 wb = t.walkB[i];
        const double4 c = t.sum[i];
        const double size = ldexp(rb.size, -wb.z);
        WalkRec r{c.x, c.y, c.z, G * c.w, (size * size) / theta2, unified(wb.x, n), unified(wb.y, n), -1, c.w > 0.0 ? 1 : 0, 0.0};   // theta = 0.5: exact
        rec[i] = r;
    }
    if (i < n) {
        const int2 lb = t.leafB[i];
        const double4 c = t.leafA[i];
        const int nx = unified(lb.x, n);
        WalkRec r{c.x, c.y, c.z, G * c.w, -1.0, nx, nx, lb.y, c.w > 0.0 ? 1 : 0, 0.0};
        rec[n - 1 + i] = r;
        leaf_of[lb.y] = i;                   // cell-sorted slot -> leaf (key order)
    }
}

// The same walk, one WAVE per 64 consecutive targets of the cell-sorted order (a column of grid cells; taking them in
// key order instead makes the union of the 64 walks 24 % larger).  The wave visits the union of its lanes' walks in the same depth-first order: the
// current node is wave-uniform (its record comes through the scalar cache, one 64-byte read for 64 lanes), every
// active lane applies its own acceptance test, and the wave descends as soon as one lane needs to.  A lane that
// accepted the node sleeps until the walk leaves that subtree -- it wakes at the node's rope, which every exit
// from the subtree reaches.  Each lane therefore accumulates exactly the contributions of its own walk, in the same
// order as grav_walk (kept as the per-lane reference implementation, SPH_GRAV_WAVE=0).
template <bool STATS>
__global__ __launch_bounds__(GB) void grav_walk_wave(int nt, int n, const WalkRec *__restrict__ rec, const double4 *__restrict__ leafA,
                                                     const double4 *__restrict__ drec, const int32_t *__restrict__ leaf_of,
                                                     const double *__restrict__ hvar,
                                                     double hfix, double soft2, double theta, double G,
                                                     const double *__restrict__ gt, int nq, double dq, double *__restrict__ ax,
                                                     double *__restrict__ ay, double *__restrict__ az, const int32_t *__restrict__ orig,
                                                     int32_t n_owned, unsigned long long *__restrict__ stats, double rb_size) {
    // nt targets (the context's cell-sorted slots); the tree has n leaves: the same particles (leaf_of: slot -> leaf),
    // or an external source set (multi-GPU: every GPU's particles; leaf_of == nullptr).  A target's own leaf needs no
    // special case then: its direction is exactly 0 and it adds 0 * f.
    const int i = xcd_chunk(blockIdx.x, gridDim.x) * GB + threadIdx.x;       // target: cell-sorted slot
    const int self = i < nt ? i : nt - 1;
    const bool live = i < nt && orig[self] < n_owned;
    const int j = leaf_of ? leaf_of[self] : -1;                               // its leaf (key order)
    const double4 p = leaf_of ? leafA[j] : drec[self];
    const double hp = hvar ? hvar[self] : hfix;
    const double inv_hp = 1.0 / hp, inv_dq = 1.0 / dq, theta2 = theta * theta, rsoft2 = 4.0 * hp * hp;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    bool active = live;                       // the root is an octree node by construction
    int resume = END;
    int node = n >= 2 ? 0 : END;
    const int own = leaf_of ? n - 1 + j : END;    // unified index of the target's own leaf
    unsigned visits = 0, sums = 0;
    // (Requesting both successors' records before the acceptance tests run -- so that the scalar-load latency overlaps the
    // tests -- changes nothing: 4.06 ms per step either way; the walk is bound by vector issue, not by the pointer chase.)
    // Per visit the walk issues ~23 vector instructions where round 2's issued 33: which lanes are awake is a 64-bit mask in scalar
    // registers (compares deliver masks, __builtin_amdgcn_fcmp / icmp; a mask predicates vector code for free, inverse_ballot), G m
    // and "has mass" come with the record, W multiplies only inside the softening support, and the softening length enters the
    // squared distance through the first fma.
    constexpr int CMP_EQ = 32, CMP_NE = 33, CMP_OLT = 4;                  // llvm::CmpInst predicates of the two builtins
    unsigned long long act_m = __builtin_amdgcn_ballot_w64(active);       // lanes walking; the others sleep until their rope (resume)
    while (node != END) {
        node = __builtin_amdgcn_readfirstlane(node);
        const WalkRec r = rec[node];
        act_m |= __builtin_amdgcn_uicmp((unsigned)resume, (unsigned)node, CMP_EQ);      // a sleeper wakes at the rope of the node it accepted
        const int n_open = r.next_open, n_skip = r.next_skip;
        const double d0 = p.x - r.cx, d1 = p.y - r.cy, d2c = p.z - r.cz;  // [F]:274
        const double d2 = fma(d2c, d2c, fma(d1, d1, fma(d0, d0, soft2)));  // [F]:275
        // [F]:278, see grav_walk: size2 holds edge^2 / theta^2 (leaves: -1, always accepted)
        const unsigned long long acc_m = __builtin_amdgcn_fcmp(r.size2, d2, CMP_OLT);
        const unsigned long long done_m = act_m & acc_m;                  // awake and satisfied with this node
        const bool open_any = (act_m & ~acc_m) != 0;                      // some awake lane has to open it
        if (r.has_mass) {
            // own leaf: direction = 0, contributes nothing
            if (__builtin_amdgcn_inverse_ballot_w64(done_m & __builtin_amdgcn_uicmp((unsigned)own, (unsigned)node, CMP_NE))) {
                const double rs = fast_rsqrt(d2);
                double f = r.gm * ((rs * rs) * rs);                       // [F]:281: G M [W] / dist^3
                if (d2 <= rsoft2) {
                    const double qi = (d2 * rs) * inv_hp;                  // dist / h
                    if (qi <= 2.0) {                                       // [F]:129-146: W = 1 beyond the softening support
                        const double tq = qi * inv_dq;
                        const int k = min((int)tq, nq - 1);
                        const double a = tq - (double)k;
                        f *= (1.0 - a) * gt[k] + a * gt[k + 1];
                    }
                }
                a0 = fma(-f, d0, a0); a1 = fma(-f, d1, a1); a2 = fma(-f, d2c, a2);
                if (STATS) sums++;
            }
        }
        if (STATS) visits++;
        if (STATS && (threadIdx.x & 63) == 0) {          // debug histogram: visits by node size (levels below the root)
            const double ratio = r.size2 > 0.0 ? r.size2 * theta2 / (rb_size * rb_size) : 0.0;
            int lv = 0;
            while (lv < 15 && ratio > 0.0 && ratio < 1.0 / (double)(1ull << (2 * lv))) lv++;
            atomicAdd(&stats[2 + (r.size2 > 0.0 ? lv : 15)], 1ull);
        }
        if (open_any) {
            resume = __builtin_amdgcn_inverse_ballot_w64(done_m) ? n_skip : resume;      // done with this subtree: sleep until its rope
            act_m &= ~done_m;
            node = n_open;
        } else {
            node = n_skip;
        }
    }
    if (live) { ax[i] = a0; ay[i] = a1; az[i] = a2; }
    if (STATS) {
        if ((threadIdx.x & 63) == 0) atomicAdd(&stats[0], (unsigned long long)visits);
        atomicAdd(&stats[1], (unsigned long long)sums);
    }
}

// phi(q) of the cubic-spline softening whose mass fraction is the grav_table polynomial ([F]:81-101): q^2 phi'(q) equals
// that polynomial, phi(q) = -1/q for q >= 2 (rq = 1/q, used only there and in the middle piece)
__device__ __forceinline__ double soft_phi(double q, double rq) {
    const double q2 = q * q;
    if (q < 1.0) return q2 * ((2.0 / 3.0) + q2 * (-0.3 + 0.1 * q)) - 1.4;
    if (q < 2.0) return (q2 * ((4.0 / 3.0) + q * (-1.0 + q * (0.3 - q * (1.0 / 30.0)))) - 1.6) + rq * (1.0 / 15.0);
    return -rq;
}

// The potential of the same Barnes-Hut walk (sph_energy): grav_walk_wave's traversal and acceptance test over the same
// records, but each accepted node or leaf of mass m adds (G m / h) phi(s / h), s = sqrt(d^2 + soft2), to the target's
// potential, and the target's own leaf is skipped by identity (it would add -1.4 G m / h, not 0).  Targets: the context's
// slots (cell-sorted: neighbouring lanes walk nearly the same nodes), owned particles only; position and h are read from
// the state fields.  The source of the target with original id k is source src_off + k, its leaf leaf_of[src_off + k].
// Writes phi[k]; never touches the accelerations.
__global__ __launch_bounds__(GB) void grav_potential_wave(int nt, int n, const WalkRec *__restrict__ rec, const double *__restrict__ x,
                                                          const double *__restrict__ y, const double *__restrict__ z,
                                                          const double *__restrict__ hvar, double hfix, double soft2,
                                                          const int32_t *__restrict__ orig, int32_t n_owned,
                                                          const int32_t *__restrict__ leaf_of, int64_t src_off, double *__restrict__ phi) {
    const int i = xcd_chunk(blockIdx.x, gridDim.x) * GB + threadIdx.x;
    const int self = i < nt ? i : nt - 1;
    const int32_t id = orig[self];
    const bool live = i < nt && id >= 0 && id < n_owned;
    const int own = live ? n - 1 + leaf_of[src_off + id] : END;
    const double px = x[self], py = y[self], pz = z[self];
    const double hp = hvar ? hvar[self] : hfix;
    const double inv_hp = 1.0 / hp;
    double acc = 0.0;
    int resume = END;
    int node = n >= 2 ? 0 : END;
    constexpr int CMP_EQ = 32, CMP_NE = 33, CMP_OLT = 4;
    unsigned long long act_m = __builtin_amdgcn_ballot_w64(live);
    while (node != END) {
        node = __builtin_amdgcn_readfirstlane(node);
        const WalkRec r = rec[node];
        act_m |= __builtin_amdgcn_uicmp((unsigned)resume, (unsigned)node, CMP_EQ);
        const int n_open = r.next_open, n_skip = r.next_skip;
        const double d0 = px - r.cx, d1 = py - r.cy, d2c = pz - r.cz;
        const double d2 = fma(d2c, d2c, fma(d1, d1, fma(d0, d0, soft2)));     // the force walk's d2 and acceptance test
        const unsigned long long acc_m = __builtin_amdgcn_fcmp(r.size2, d2, CMP_OLT);
        const unsigned long long done_m = act_m & acc_m;
        const bool open_any = (act_m & ~acc_m) != 0;
        if (r.has_mass) {
            if (__builtin_amdgcn_inverse_ballot_w64(done_m & __builtin_amdgcn_uicmp((unsigned)own, (unsigned)node, CMP_NE))) {
                const double rs = fast_rsqrt(d2);                  // 1 / s
                const double q = (d2 * rs) * inv_hp;               // s / h
                acc += (r.gm * inv_hp) * soft_phi(q, hp * rs);
            }
        }
        if (open_any) {
            resume = __builtin_amdgcn_inverse_ballot_w64(done_m) ? n_skip : resume;
            act_m &= ~done_m;
            node = n_open;
        } else {
            node = n_skip;
        }
    }
    if (live) phi[id] = acc;
}

// gamma(q) = M(q) / q^3 inside the softening support, M the grav_table polynomial ([F]:81-101) divided analytically (finite
// at q = 0); rq = 1 / q, used in the middle piece only.  phi'(q) = q gamma(q): the pull that belongs to soft_phi.
__device__ __forceinline__ double soft_gamma(double q, double rq) {
#pragma clang fp contract(off)
    if (q < 1.0) return (4.0 / 3.0) + (q * q) * (-1.2 + 0.5 * q);
    return ((8.0 / 3.0) + q * (-3.0 + q * (1.2 - q * (1.0 / 6.0)))) - ((rq * rq) * rq) * (1.0 / 15.0);
}

// The field of the same Barnes-Hut walk at points that are not particles (sph_gravity_at): grav_potential_wave's traversal,
// acceptance test and sleeping lanes over the same records, one wave per 64 points of the walk order (pidx: the points
// sorted by their path key, or null: the caller's order).  Each accepted node or leaf of mass m adds, with
// s = sqrt(d^2 + soft2) and q = s / h_p,
//   q < 2:   Phi += (G m / h_p) phi(q),  a -= ((G m / h_p^3) gamma(q)) d
//   q >= 2:  Phi -= (G m) (1 / s),       a -= ((G m) (1 / s)^3) d
// Points are not sources: nothing is excluded, and s = 0 (a point on a source, soft2 = 0) is q = 0, finite.  Dead lanes
// (the tail, a non-finite coordinate, h <= 0 or non-finite) never wake and write nothing.  A lane's arithmetic does not
// depend on the other lanes, so a point's rows do not depend on its neighbours in the wave.  (A wave-uniform test "every
// contributing lane has q >= 2" that skips the softening branch altogether measured 4 % slower, 1.95 against 1.88 ms for
// 10^6 points: the branch is already skipped by the lanes' own compare, and the mask costs a scalar round trip per visit.)
// Writes the four rows out[c * m + point], c = 0 Phi, 1..3 a, with plain stores.
__global__ __launch_bounds__(GB) void grav_field_points(int64_t m, int n, const WalkRec *__restrict__ rec, const double *__restrict__ px,
                                                        const double *__restrict__ py, const double *__restrict__ pz,
                                                        const double *__restrict__ ph, double hfix, double soft2,
                                                        const uint32_t *__restrict__ pidx, double *__restrict__ out) {
#pragma clang fp contract(off)
    const int64_t t = (int64_t)xcd_chunk(blockIdx.x, gridDim.x) * GB + threadIdx.x;
    const int64_t tc = t < m ? t : m - 1;
    const int64_t idx = pidx ? (int64_t)pidx[tc] : tc;
    const double x = px[idx], y = py[idx], z = pz[idx];
    const double hp = ph ? ph[idx] : hfix;
    constexpr double BIG = 1.7976931348623157e308;
    const bool live = t < m && fabs(x) <= BIG && fabs(y) <= BIG && fabs(z) <= BIG && hp > 0.0 && hp <= BIG;
    const double inv_hp = 1.0 / hp;
    const double inv_hp3 = (inv_hp * inv_hp) * inv_hp;
    double phi = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0;
    int resume = END;
    int node = n >= 1 ? 0 : END;                  // one source: its leaf is record 0 and ends the walk
    constexpr int CMP_EQ = 32, CMP_OLT = 4;
    unsigned long long act_m = __builtin_amdgcn_ballot_w64(live);
    while (node != END) {
        node = __builtin_amdgcn_readfirstlane(node);
        const WalkRec r = rec[node];
        act_m |= __builtin_amdgcn_uicmp((unsigned)resume, (unsigned)node, CMP_EQ);
        const int n_open = r.next_open, n_skip = r.next_skip;
        const double d0 = x - r.cx, d1 = y - r.cy, d2c = z - r.cz;
        const double d2 = fma(d2c, d2c, fma(d1, d1, fma(d0, d0, soft2)));     // the force walk's d2 and acceptance test
        const unsigned long long acc_m = __builtin_amdgcn_fcmp(r.size2, d2, CMP_OLT);
        const unsigned long long done_m = act_m & acc_m;
        const bool open_any = (act_m & ~acc_m) != 0;
        if (r.has_mass) {
            if (__builtin_amdgcn_inverse_ballot_w64(done_m)) {
                const double rs = d2 > 0.0 ? fast_rsqrt(d2) : 0.0;            // 1 / s (unused at s = 0)
                const double q = (d2 * rs) * inv_hp;                          // s / h
                double pt = -(r.gm * rs), f = r.gm * ((rs * rs) * rs);        // q >= 2
                if (q < 2.0) {
                    const double rq = hp * rs;
                    pt = (r.gm * inv_hp) * soft_phi(q, rq);
                    f = (r.gm * inv_hp3) * soft_gamma(q, rq);
                }
                phi += pt;
                a0 = fma(-f, d0, a0); a1 = fma(-f, d1, a1); a2 = fma(-f, d2c, a2);
            }
        }
        if (open_any) {
            resume = __builtin_amdgcn_inverse_ballot_w64(done_m) ? n_skip : resume;
            act_m &= ~done_m;
            node = n_open;
        } else {
            node = n_skip;
        }
    }
    if (live) {
        out[idx] = phi; out[m + idx] = a0; out[2 * m + idx] = a1; out[3 * m + idx] = a2;
    }
}

}  // namespace

hipError_t grav_sort_tmp_bytes(int64_t n, size_t *bytes) {
    size_t b = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (size_t)n, 0u, 63u, (hipStream_t) nullptr);
    *bytes = b;
    return e;
}

static TreeArrays tree_arrays(sph_ctx *c) {
    TreeArrays t;
    t.left = c->g_left; t.right = c->g_right; t.parent = c->g_parent; t.leaf_parent = c->g_leaf_parent; t.prefix = c->g_prefix;
    t.other = c->g_flag; t.seg = reinterpret_cast<double4 *>(c->g_seg); t.sum = reinterpret_cast<double4 *>(c->g_sum); t.leafA = reinterpret_cast<double4 *>(c->g_leafA);
    t.slot = c->g_slot; t.lvl = c->g_lvl; t.rope = c->g_rope; t.leaf_rope = c->g_leaf_rope;
    t.walkB = reinterpret_cast<int4 *>(c->g_walkB); t.leafB = reinterpret_cast<int2 *>(c->g_leafB);
    return t;
}

void gravity_free(sph_ctx *c) {
    ctx_free(c, c->g_left); ctx_free(c, c->g_right); ctx_free(c, c->g_parent); ctx_free(c, c->g_leaf_parent);
    ctx_free(c, c->g_prefix); ctx_free(c, c->g_flag); ctx_free(c, c->g_slot); ctx_free(c, c->g_lvl); ctx_free(c, c->g_rope);
    ctx_free(c, c->g_leaf_rope); ctx_free(c, c->g_sum); ctx_free(c, c->g_seg); ctx_free(c, c->g_wrec); ctx_free(c, c->g_leaf_of);
    ctx_free(c, c->g_leafA); ctx_free(c, c->g_walkB); ctx_free(c, c->g_leafB);
    ctx_free(c, c->g_keys); ctx_free(c, c->g_keys_alt); ctx_free(c, c->g_vals); ctx_free(c, c->g_vals_alt);
    ctx_free_ptr(c, c->g_sort_tmp); c->g_sort_tmp = nullptr; c->g_sort_tmp_bytes = 0;
    c->g_cap = 0; c->tree_arrays_freed();
}

// tree arrays for `need` leaves (the context's slots, or an external source set that may be much larger)
static int gravity_reserve(sph_ctx *c, int64_t need) {
    if (need <= c->g_cap) return SPH_OK;
    gravity_free(c);
    const size_t cap = (size_t)(need + need / 16 + 64);
#define G_ALLOC(p, cnt, what) do { int _s = ctx_alloc(c, &(p), (cnt), what); if (_s != SPH_OK) return _s; } while (0)
    G_ALLOC(c->g_left, cap, "tree left"); G_ALLOC(c->g_right, cap, "tree right"); G_ALLOC(c->g_parent, cap, "tree parent");
    G_ALLOC(c->g_leaf_parent, cap, "leaf parent"); G_ALLOC(c->g_prefix, cap, "tree prefix"); G_ALLOC(c->g_flag, cap, "range ends");
    G_ALLOC(c->g_slot, cap, "leaf slots"); G_ALLOC(c->g_lvl, cap, "tree levels"); G_ALLOC(c->g_rope, cap, "tree ropes");
    G_ALLOC(c->g_leaf_rope, cap, "leaf ropes"); G_ALLOC(c->g_sum, cap * 4, "node sums"); G_ALLOC(c->g_seg, (cap + 64) * 4, "segment tree");
    G_ALLOC(c->g_wrec, cap * 16, "wave walk records"); G_ALLOC(c->g_leaf_of, cap, "slot -> leaf"); G_ALLOC(c->g_leafA, cap * 4, "leaf records");
    G_ALLOC(c->g_walkB, cap * 4, "walk records"); G_ALLOC(c->g_leafB, cap * 2, "leaf walk records");
    G_ALLOC(c->g_keys, cap, "tree keys"); G_ALLOC(c->g_keys_alt, cap, "tree keys (alt)");
    G_ALLOC(c->g_vals, cap, "tree vals"); G_ALLOC(c->g_vals_alt, cap, "tree vals (alt)");
#undef G_ALLOC
    size_t tmp = 0;
    SPH_HIP(grav_sort_tmp_bytes((int64_t)cap, &tmp));
    if (ctx_alloc_bytes(c, &c->g_sort_tmp, tmp ? tmp : 1, "tree sort scratch") != SPH_OK) return SPH_ERR_NOMEM;
    c->g_sort_tmp_bytes = tmp;
    c->g_cap = (int64_t)cap;
    return SPH_OK;
}

// path keys of the external source set, sorted (shared by the gravity tree, the variable-h leaf boxes and accretion)
int global_keys_sorted(sph_ctx *c) {
    if (!c->gx_src) { c->err = "no external source set"; return SPH_ERR_STATE; }
    if (c->gx_keys_valid) return SPH_OK;
    const int64_t n = c->gx_n;
    { const int st = gravity_reserve(c, n); if (st != SPH_OK) return st; }
    RootBox rb;
    double size = 0.0;
    for (int a = 0; a < 3; a++) {
        rb.c[a] = (c->gx_box[3 + a] + c->gx_box[a]) / 2.0;
        size = std::max(size, c->gx_box[3 + a] - c->gx_box[a]);
    }
    rb.size = size;
    grav_keys<<<dim3((unsigned)((n + GB - 1) / GB)), dim3(GB), 0, c->stream>>>(rb, reinterpret_cast<const double4 *>(c->gx_src), n, c->g_keys, c->g_vals);
    SPH_HIP(hipGetLastError());
    size_t tmp = c->g_sort_tmp_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(c->g_sort_tmp, tmp, c->g_keys, c->g_keys_alt, c->g_vals, c->g_vals_alt, (size_t)n, 0u, 63u, c->stream));
    c->gx_keys_valid = true;
    return SPH_OK;
}

// the tree over n sources whose sorted path keys are in g_keys_alt / g_vals_alt: leaves, radix tree, node sums, walk records
static int tree_from_sorted_keys(sph_ctx *c, const double4 *drec, int64_t n, const RootBox &rb) {
    const unsigned gb = (unsigned)((n + GB - 1) / GB);
    TreeArrays t = tree_arrays(c);
    leaf_data<<<dim3(gb), dim3(GB), 0, c->stream>>>(c->g_vals_alt, drec, (int)n, t);
    if (n >= 2) {
        radix_tree<<<dim3(gb), dim3(GB), 0, c->stream>>>(c->g_keys_alt, (int)n, t);
        SegLevels sl{};
        sl.cnt[0] = n; sl.off[0] = 0; sl.levels = 1;
        int64_t off = 0;
        while (sl.cnt[sl.levels - 1] > 1 && sl.levels < SEG_MAX_LEVELS) {
            sl.cnt[sl.levels] = (sl.cnt[sl.levels - 1] + 1) / 2;
            sl.off[sl.levels] = off;
            off += sl.cnt[sl.levels];
            sl.levels++;
        }
        for (int L0 = 0; L0 + 1 < sl.levels; L0 += SEG_LV)
            seg_stage<<<dim3((unsigned)((sl.cnt[L0] + 511) / 512)), dim3(256), 0, c->stream>>>(sl, L0, t.leafA, t.seg);
        node_sums_seg<<<dim3(gb), dim3(GB), 0, c->stream>>>((int)n, sl, t);
    }
    node_finish<<<dim3(gb), dim3(GB), 0, c->stream>>>((int)n, t);
    node_walk_records<<<dim3(gb), dim3(GB), 0, c->stream>>>((int)n, t);
    node_wave_records<<<dim3(gb), dim3(GB), 0, c->stream>>>((int)n, t, rb, c->p.theta * c->p.theta, c->p.G, reinterpret_cast<WalkRec *>(c->g_wrec), c->g_leaf_of);
    SPH_HIP(hipGetLastError());
    return SPH_OK;
}

// root box of a source set: bbox-midpoint centre, edge = largest extent ([F]:803-808)
static RootBox root_of(const double *bb) {
    RootBox rb;
    double size = 0.0;
    for (int a = 0; a < 3; a++) {
        rb.c[a] = (bb[3 + a] + bb[a]) / 2.0;
        size = std::max(size, bb[3 + a] - bb[a]);
    }
    rb.size = size;
    return rb;
}

// builds the tree over the context's own particles (current cell-sorted positions) or over the external source set
int gravity_tree_build(sph_ctx *c) {
    const bool ext = c->gx_src != nullptr;
    const int64_t n = ext ? c->gx_n : c->n;
    if (n == 0) return SPH_OK;
    if (n > 2000000000LL) { c->err = "gravity: more than 2e9 sources"; return SPH_ERR_ARG; }
    { const int st = gravity_reserve(c, ext ? n : std::max(c->cap, n)); if (st != SPH_OK) return st; }
    const RootBox rb = root_of(ext ? c->gx_box : c->bbox);
    for (int a = 0; a < 3; a++) c->root_box[a] = rb.c[a];
    c->root_box[3] = rb.size;
    const unsigned gb = (unsigned)((n + GB - 1) / GB);
    const double4 *drec = reinterpret_cast<const double4 *>(ext ? c->gx_src : c->drec);
    if (ext) {
        const int st = global_keys_sorted(c);
        if (st != SPH_OK) return st;
    } else {
        if (c->path_keys_valid && c->mkeys_alt && c->mvals_alt) {
            // variable h: the leaf-box build of this grid build sorted the same keys (same positions, same root box)
            SPH_HIP(hipMemcpyAsync(c->g_keys_alt, c->mkeys_alt, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
            SPH_HIP(hipMemcpyAsync(c->g_vals_alt, c->mvals_alt, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        } else {
            grav_keys<<<dim3(gb), dim3(GB), 0, c->stream>>>(rb, drec, n, c->g_keys, c->g_vals);
            SPH_HIP(hipGetLastError());
            size_t tmp = c->g_sort_tmp_bytes;
            SPH_HIP(rocprim::radix_sort_pairs(c->g_sort_tmp, tmp, c->g_keys, c->g_keys_alt, c->g_vals, c->g_vals_alt, (size_t)n, 0u, 63u, c->stream));
        }
    }
    return tree_from_sorted_keys(c, drec, n, rb);
}

// sph_energy: the tree over n caller-given {x, y, z, m} records in their order and their box -- the tree that
// gravity_tree_build makes of an external source set with the same records and box (the same keys, the same stable
// sort, the same kernels).  Built into the context's tree arrays: the context's own tree, the sorted external keys
// and the cached self-gravity term are no longer there, so they are marked stale (the next sph_forces rebuilds them).
int gravity_tree_build_records(sph_ctx *c, const double *rec, int64_t n, const double box[6]) {
    c->tree_arrays_taken();
    if (n == 0) return SPH_OK;
    if (n > 2000000000LL) { c->err = "gravity: more than 2e9 sources"; return SPH_ERR_ARG; }
    { const int st = gravity_reserve(c, std::max(c->cap, n)); if (st != SPH_OK) return st; }
    const RootBox rb = root_of(box);
    const double4 *drec = reinterpret_cast<const double4 *>(rec);
    grav_keys<<<dim3((unsigned)((n + GB - 1) / GB)), dim3(GB), 0, c->stream>>>(rb, drec, n, c->g_keys, c->g_vals);
    SPH_HIP(hipGetLastError());
    size_t tmp = c->g_sort_tmp_bytes;
    SPH_HIP(rocprim::radix_sort_pairs(c->g_sort_tmp, tmp, c->g_keys, c->g_keys_alt, c->g_vals, c->g_vals_alt, (size_t)n, 0u, 63u, c->stream));
    return tree_from_sorted_keys(c, drec, n, rb);
}

// sph_energy: the self-potential of every owned particle by the walk over the tree in place (n_src leaves; source
// src_off + k is the particle of original id k) -> phi[k], k < n_owned
hipError_t launch_potential(sph_ctx *c, int64_t n_src, int64_t src_off, double *phi) {
    const int64_t nt = c->n_slots;
    if (nt == 0 || n_src == 0 || c->n_owned == 0) return hipSuccess;
    const double soft2 = 0.001 * 2.5;                                   // as launch_gravity
    grav_potential_wave<<<dim3((unsigned)((nt + GB - 1) / GB)), dim3(GB), 0, c->stream>>>(
        (int)nt, (int)n_src, reinterpret_cast<const WalkRec *>(c->g_wrec), c->f[SPH_F_X], c->f[SPH_F_Y], c->f[SPH_F_Z],
        c->variable ? c->f[SPH_F_H] : nullptr, c->p.h, soft2, c->orig, (int32_t)c->n_owned, c->g_leaf_of, src_off, phi);
    return hipGetLastError();
}

// sph_gravity_at: Phi and a of the tree in place (n_src >= 1 leaves) at m points -> out[c * m + p], c < 4; ph: the points'
// softening lengths or null (h_one for all); pidx: the walk order or null
hipError_t launch_field_points(sph_ctx *c, int64_t n_src, int64_t m, const double *px, const double *py, const double *pz,
                               const double *ph, double h_one, double soft2, const uint32_t *pidx, double *out) {
    if (m == 0 || n_src == 0) return hipSuccess;
    grav_field_points<<<dim3((unsigned)((m + GB - 1) / GB)), dim3(GB), 0, c->stream>>>(
        m, (int)n_src, reinterpret_cast<const WalkRec *>(c->g_wrec), px, py, pz, ph, h_one, soft2, pidx, out);
    return hipGetLastError();
}

// ax, ay, az: where the term goes, slot order (null: the context's SPH_F_AX..AZ, what sph_forces continues from;
// sph_force_terms gives its own scratch and leaves the fields alone)
hipError_t launch_gravity(sph_ctx *c, double *ax, double *ay, double *az) {
    if (!ax) { ax = c->f[SPH_F_AX]; ay = c->f[SPH_F_AY]; az = c->f[SPH_F_AZ]; }
    const bool ext = c->gx_src != nullptr;
    const int64_t nt = c->n;                     // targets: the context's slots
    const int64_t n = ext ? c->gx_n : c->n;      // leaves of the tree
    if (nt == 0 || n == 0) return hipSuccess;
    RootBox rb;
    for (int a = 0; a < 3; a++) rb.c[a] = c->root_box[a];
    rb.size = c->root_box[3];
    const double soft2 = 0.001 * 2.5;                                   // 0.001_dp*smoothing, MODULE constant ([F]:275, [V]:296)
    const int wave_walk = switches().grav_wave;                         // SPH_GRAV_WAVE: A/B switch
    if (wave_walk || ext) {
        TreeArrays ta = tree_arrays(c);
        unsigned long long *stats = nullptr;
        if (wave_walk == 2) {                                           // debug: visit / contribution counts
            if (hipMalloc(reinterpret_cast<void **>(&stats), 18 * 8) != hipSuccess) return hipGetLastError();
            (void)hipMemsetAsync(stats, 0, 18 * 8, c->stream);
        }
        auto walk = stats ? grav_walk_wave<true> : grav_walk_wave<false>;
        walk<<<dim3((unsigned)((nt + GB - 1) / GB)), dim3(GB), 0, c->stream>>>(
            (int)nt, (int)n, reinterpret_cast<const WalkRec *>(c->g_wrec), ta.leafA, reinterpret_cast<const double4 *>(c->drec),
            ext ? nullptr : c->g_leaf_of, c->variable ? c->f[SPH_F_H] : nullptr, c->p.h, soft2,
            c->p.theta, c->p.G, c->grav_tab, c->p.nq, 2.0 / c->p.nq, ax, ay, az, c->orig,
            (int32_t)c->n_owned, stats, rb.size);
        if (stats) {
            unsigned long long h[18] = {0};
            (void)hipStreamSynchronize(c->stream);
            (void)hipMemcpy(h, stats, 18 * 8, hipMemcpyDeviceToHost);
            fprintf(stderr, "[grav_walk_wave] visits per wave by level (0..14, leaves):");
            for (int k = 0; k < 16; k++) fprintf(stderr, " %.1f", (double)h[2 + k] / (double)((nt + 63) / 64));
            fprintf(stderr, "\n");
            (void)hipFree(stats);
            fprintf(stderr, "[grav_walk_wave] n=%lld wave visits/wave=%.1f contributions/particle=%.1f\n", (long long)n,
                    (double)h[0] / (double)((n + 63) / 64), (double)h[1] / (double)n);
        }
        return hipGetLastError();
    }
    grav_walk<<<dim3((unsigned)((n + GB - 1) / GB)), dim3(GB), 0, c->stream>>>(
        (int)n, tree_arrays(c), rb, reinterpret_cast<const double4 *>(c->drec), c->variable ? c->f[SPH_F_H] : nullptr, c->p.h, soft2,
        c->p.theta, c->p.G, c->grav_tab, c->p.nq, 2.0 / c->p.nq, ax, ay, az, c->orig,
        (int32_t)c->n_owned);
    return hipGetLastError();
}

}  // namespace sph
