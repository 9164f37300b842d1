// fd2_map_part.hip -- per-base launchers of the unique-count map kernel
// (fd2_map_kernel, fd2_map_kernel.hpp), one object per part like fd2_part.hip
// (built with -DFD2_PART=k, k < FD2_NPARTS): objects of their own, so the
// field and batch kernels' objects are built from the text they always were.
#include "fd2_combos.h"
#include "fd2_launch.hpp"
#include "fd2_map_kernel.hpp"

#ifndef FD2_PART
#error "build with -DFD2_PART=k"
#endif

#define FD2_CAT2(a, b) a##b
#define FD2_CAT(a, b) FD2_CAT2(a, b)

namespace nice {
namespace fd2 {

// One map launch: `n` descriptors (all of this P's combo) from `units`.
template <class P>
static hipError_t launch_map_cfg(const Fd2MapUnit *units, u32 n, unsigned char *out, hipStream_t s) {
    const uint4 *tabs = nullptr;
    hipError_t e = fd2_tables<P>(s, &tabs);
    if (e != hipSuccess) return e;
    Fd2MapArgs a{};
    a.units = units;
    a.out = out;
    a.tabs = tabs;
    hipLaunchKernelGGL(fd2_map_kernel<P>, dim3(n), dim3(P::WG), 0, s, a);
    return hipGetLastError();
}

// hipErrorNotFound: not this part's (base, combo).
hipError_t FD2_CAT(launch_map_part, FD2_PART)(uint32_t base, int nd, int ne, int ne2, const void *units,
                                              uint32_t n, unsigned char *out, hipStream_t s) {
#define X(B_, ND_, NE_, NE2_)                                                                  \
    if constexpr (fd2_part_of(B_) == FD2_PART) {                                               \
        if ((int)base == B_ && nd == ND_ && ne == NE_ && ne2 == NE2_)                          \
            return launch_map_cfg<MapCfg<B_, ND_, NE_, NE2_>>((const Fd2MapUnit *)units, n, out, s); \
    }
    FD2_COMBOS(X)
#undef X
    return hipErrorNotFound;
}

}  // namespace fd2
}  // namespace nice
