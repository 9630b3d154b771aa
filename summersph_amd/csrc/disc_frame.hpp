// disc_frame.hpp -- the disc frame of sph_profile and sph_modes (profile.hip, modes.hip): the centre (given, or a sink's
// state on the device), the axes e1, e2, n^ built from a normal on the host, a particle's position in that frame, and the
// ring edge table.  One definition, so that both calls select and place a particle by the same arithmetic.
#pragma once
#include <cmath>

#include "sph_internal.hpp"

// the per-particle arithmetic is written in one documented order (summersph.h); no contraction into fused multiply-adds,
// so that a numpy restatement reproduces it.  (File scope: it also holds for the rest of the including file, which states
// it again for itself.)
#pragma clang fp contract(off)

namespace sph {

struct DiscFrame {
    double c[3], cv[3];            // centre and its velocity (sink < 0)
    double e1[3], e2[3], n[3];     // frame axes, lab components
    double cm;                     // central mass (sink < 0)
    double G;
    double fixed_h;                // h of every particle when hf is null
    const double *sink;            // the context's sink arrays (x y z vx vy vz m, MAX_SINKS each)
    const double *hf;              // per-particle h (variable h) or null
    int32_t sink_k;                // >= 0: centre, centre velocity and central mass are this sink's
};

__device__ __forceinline__ void centre_of(const DiscFrame &f, double c[3], double cv[3], double &cm) {
    if (f.sink_k >= 0) {
        for (int a = 0; a < 3; a++) { c[a] = f.sink[a * MAX_SINKS + f.sink_k]; cv[a] = f.sink[(3 + a) * MAX_SINKS + f.sink_k]; }
        cm = f.sink[6 * MAX_SINKS + f.sink_k];
    } else {
        for (int a = 0; a < 3; a++) { c[a] = f.c[a]; cv[a] = f.cv[a]; }
        cm = f.cm;
    }
}

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// r' = r - c, X = r'.e1, Y = r'.e2, z' = r'.n, R = sqrt(X^2 + Y^2)
struct Pos { double r[3], X, Y, Z, R; };

__device__ __forceinline__ Pos frame_pos(const DiscFrame &f, const double c[3], double x, double y, double z) {
    Pos p;
    p.r[0] = x - c[0]; p.r[1] = y - c[1]; p.r[2] = z - c[2];
    p.X = dot3(p.r, f.e1); p.Y = dot3(p.r, f.e2); p.Z = dot3(p.r, f.n);
    p.R = sqrt(p.X * p.X + p.Y * p.Y);
    return p;
}

// n^ = n / |n|; a = x^ if |n^_x| <= 0.9 else y^; e1 = normalise(a - (a.n^) n^); e2 = n^ x e1.  false: the normal cannot be
// normalised (zero or not finite)
inline bool frame_axes(const double nin[3], double n[3], double e1[3], double e2[3]) {
    const double len = std::sqrt((nin[0] * nin[0] + nin[1] * nin[1]) + nin[2] * nin[2]);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    for (int a = 0; a < 3; a++) n[a] = nin[a] / len;
    double av[3] = {0.0, 0.0, 0.0};
    av[std::fabs(n[0]) <= 0.9 ? 0 : 1] = 1.0;
    const double an = (av[0] * n[0] + av[1] * n[1]) + av[2] * n[2];
    double t[3];
    for (int a = 0; a < 3; a++) t[a] = av[a] - an * n[a];
    const double tl = std::sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    for (int a = 0; a < 3; a++) e1[a] = t[a] / tl;
    e2[0] = n[1] * e1[2] - n[2] * e1[1];
    e2[1] = n[2] * e1[0] - n[0] * e1[2];
    e2[2] = n[0] * e1[1] - n[1] * e1[0];
    return true;
}

// edge[k], k in [0, n_r]: linear r_min + k (r_max - r_min) / n_r, log r_min (r_max / r_min)^(k / n_r); edge[n_r] = r_max
inline void ring_edge_table(double r_min, double r_max, int nr, bool lg, double *edge) {
    for (int k = 0; k < nr; k++)
        edge[k] = lg ? r_min * std::pow(r_max / r_min, (double)k / (double)nr) : r_min + ((double)k * (r_max - r_min)) / (double)nr;
    edge[nr] = r_max;
}

}  // namespace sph
