// region_index.h -- the ONE statement of the geometric half of the resident batch's augmentation, shared by the kernels that assemble the
// batch (region_batch.hip) and the kernel that patches it afterwards (region_repair.hip), so that the two cannot drift:
//
//   out = rot90^rot( hflip( vflip( T ) ) )          T the gathered tile (Hm x Wm), out (Ho x Wo) = (Wm x Hm) for an odd rot
//
// pc_region_out_to_tile gives the tile position (y, x) an output position (i, j) shows; pc_region_tile_to_out is its inverse.  A half turn
// mirrors both axes and a flip mirrors one, so for an even rot the map is a mirror per axis: pc_region_yrev / pc_region_xrev.
#pragma once
#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ bool pc_region_yrev(int vflip, int rot) { return ((rot & 2) != 0) != (vflip != 0); }
__host__ __device__ __forceinline__ bool pc_region_xrev(int hflip, int rot) { return ((rot & 2) != 0) != (hflip != 0); }

__host__ __device__ __forceinline__ void pc_region_out_to_tile(int i, int j, int Hm, int Wm, int vflip, int hflip, int rot, int& y, int& x) {
    switch (rot & 3) {
        case 0: y = i; x = j; break;
        case 1: y = j; x = Wm - 1 - i; break;
        case 2: y = Hm - 1 - i; x = Wm - 1 - j; break;
        default: y = Hm - 1 - j; x = i; break;
    }
    if (hflip) x = Wm - 1 - x;
    if (vflip) y = Hm - 1 - y;
}

__host__ __device__ __forceinline__ void pc_region_tile_to_out(int y, int x, int Hm, int Wm, int vflip, int hflip, int rot, int& i, int& j) {
    if (vflip) y = Hm - 1 - y;
    if (hflip) x = Wm - 1 - x;
    switch (rot & 3) {
        case 0: i = y; j = x; break;
        case 1: j = y; i = Wm - 1 - x; break;
        case 2: i = Hm - 1 - y; j = Wm - 1 - x; break;
        default: j = Hm - 1 - y; i = x; break;
    }
}
