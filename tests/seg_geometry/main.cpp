// Prints what csrc/sgcn_seg.h derives, for tests/test_seg_geometry.py: the lane geometry over a grid of (nvec, nv_force, nseg),
// the rungs with_gnv accepts with the constants it hands on, and the width with_vw picks.  Plain C++: no HIP, no device.
#include <cstdio>
#include "sgcn_seg.h"

namespace sgcn {
char* error_slot() { static char slot[512]; return slot; }
}  // namespace sgcn

int main() {
    using namespace sgcn;
    const long long nsegs[] = {0, 1, 31, 32, 33, 4097};
    for (int nvec = 1; nvec <= 1100; nvec++)
        for (int nv_force = 0; nv_force <= 4; nv_force++)
            for (long long nseg : nsegs) {
                const SegGeom g = seg_geometry(nvec, nseg, nv_force);
                printf("geom %d %d %lld %d %d %d %lld %lld\n", nvec, nv_force, nseg, g.G, g.NV, g.nslab, (long long)g.nsegblk,
                       (long long)g.nblocks);
            }
    for (int G = 0; G <= 130; G++)
        for (int NV = 0; NV <= 6; NV++) {
            int g = -1, nv = -1, calls = 0;
            const bool ok = with_gnv(G, NV, [&](auto cg, auto cnv) { g = decltype(cg)::value; nv = decltype(cnv)::value; calls++; });
            printf("gnv %d %d %d %d %d %d\n", G, NV, (int)ok, calls, g, nv);
        }
    for (int vw = 0; vw <= 8; vw++) printf("vw %d %d\n", vw, with_vw(vw, [](auto cvw) { return (int)decltype(cvw)::value; }));
    printf("pitch");
    for (int d = 1; d <= 9; d++) printf(" %lld", (long long)seg_slot_pitch(d));
    printf("\nfix %lld %lld %lld\n", (long long)seg_fix_blocks(256, 3), (long long)seg_fix_blocks(257, 3),
           (long long)seg_fix_blocks(1, 1ll << 31));
    return 0;
}
