// gsr_volume.h -- the dense directory of 16^3-voxel units that gsr_fusion.hip and gsr_hull.hip share: the [host] grid block
// (first unit index and units along x, y, z) and its checks.  Arrays over it are [nz,ny,nx], x fastest; unit (ux, uy, uz) has
// the index (uz nu_y + uy) nu_x + ux; voxel k of a unit along an axis has its centre at (u0 + u) L + (k + 0.5) voxel, L = 16 voxel,
// formed in double in exactly that order.
#pragma once

namespace gsr {

namespace {

constexpr int FU = 16;                       // voxels along a unit's edge (ScalableTSDFVolume's volume_unit_resolution)
constexpr int FU_QUADS = FU * FU * FU / 4;   // float4 per unit and plane

struct FusionGrid {
    int u0[3];   // unit index (floor(p / L)) of the first unit along x, y, z
    int nu[3];   // units along x, y, z
};

inline FusionGrid fusion_grid(const int* grid6)
{
    FusionGrid g;
    for (int a = 0; a < 3; ++a) { g.u0[a] = grid6[a]; g.nu[a] = grid6[3 + a]; }
    return g;
}

// the [host] grid block of the fusion calls: a directory of at least one unit per axis whose voxels can be counted in an int
inline const char* fusion_grid_error(const int* grid)
{
    if (!grid) return "grid is null";
    long long units = 1;
    for (int a = 0; a < 3; ++a) {
        if (grid[3 + a] <= 0 || grid[3 + a] > (1 << 16)) return "units per axis must be in [1, 65536]";
        if (grid[a] < -(1 << 24) || grid[a] > (1 << 24)) return "first unit index out of range";
        units *= grid[3 + a];
    }
    return units * 4096 >= (1ll << 31) ? "the volume has 2^31 voxels or more" : nullptr;
}

}  // namespace

}  // namespace gsr
