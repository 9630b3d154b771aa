"""CPU test of what csrc/exact_sum.hpp shares on the host: hist_plan, the sizing of the LDS limb histogram of pairs_bin
(sph_pairs) and modes_rings (sph_modes), through a stand-alone host program, for every (segments, accumulators per segment)
the two descriptors allow."""
import subprocess

import numpy as np

from abi_support import CSRC, HIPCC, hipcc_flags, needs_hipcc

HIST, MAX_COPIES, SLAB_BYTES = 3072, 8, 64 << 20
CAPS = (1, 3, 100, 512)                          # the callers' caps: BIN_BLOCKS = RING_BLOCKS = 512, or the fewer blocks n_slots gives

PROGRAM = r"""
#include <cstdio>
#include "exact_sum.hpp"
int main() {
    using namespace sph;
    const long caps[] = {%s};
    for (long cap : caps) {
        for (int q = 0; q <= SPH_PAIRS_MAX_Q; q++)
            for (int v = 0; v < 2; v++)
                for (int n = 1; n <= SPH_PAIRS_MAX_BINS; n++) {
                    const int na = 2 + 2 * q + 4 * v;
                    const HistPlan p = hist_plan<2 + 2 * SPH_PAIRS_MAX_Q + 4>(n, na, cap);
                    std::printf("%%d %%d %%ld %%d %%d %%d\n", n, na, cap, p.chunk, p.copies, p.nslab);
                }
        for (int m = 0; m <= SPH_MODES_MAX_M; m++)
            for (int n = 1; n <= SPH_MODES_MAX_RINGS; n++) {
                const int na = 2 * (m + 1) + 1;
                const HistPlan p = hist_plan<2 * (SPH_MODES_MAX_M + 1) + 1>(n, na, cap);
                std::printf("%%d %%d %%ld %%d %%d %%d\n", n, na, cap, p.chunk, p.copies, p.nslab);
            }
    }
    return 0;
}
"""


@needs_hipcc
def test_histogram_sizing_for_every_descriptor(tmp_path):
    src, exe = tmp_path / "plan.hip", tmp_path / "plan"
    src.write_text(PROGRAM % ", ".join(str(b) for b in CAPS))
    subprocess.run([HIPCC, *hipcc_flags(), "--offload-host-only", "-I", CSRC, str(src), "-o", str(exe)], check=True,
                   capture_output=True)
    rows = np.array(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split(), dtype=np.int64)
    segs, na, cap, chunk, copies, nslab = rows.reshape(-1, 6).T
    per_cap = 10 * 1024 + 9 * 1024               # sph_pairs: n_q 0 .. 4 with and without velocity; sph_modes: m_max 0 .. 8
    assert len(segs) == len(CAPS) * per_cap
    assert set(na[:10 * 1024]) == {2, 4, 6, 8, 10, 12, 14} and set(na[10 * 1024:per_cap]) == set(range(3, 20, 2))
    assert np.all((1 <= chunk) & (chunk <= segs))
    assert np.all((1 <= copies) & (copies <= MAX_COPIES))
    assert np.all(chunk * na * copies <= HIST)
    # the formulas of the two calls as they stood in pair_stats.hip and modes.hip
    want_chunk = np.minimum(segs, HIST // na)
    want_copies = np.maximum(1, np.minimum(MAX_COPIES, HIST // (want_chunk * na)))
    want_nslab = np.maximum(1, np.minimum(cap, SLAB_BYTES // (segs * na * 16)))
    assert np.array_equal(chunk, want_chunk) and np.array_equal(copies, want_copies) and np.array_equal(nslab, want_nslab)
    assert chunk.min() < segs.max() and copies.min() == 1 and copies.max() == MAX_COPIES      # one chunk and several, 1 and 8 copies
