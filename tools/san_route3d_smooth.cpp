// Stand-alone driver of the volume smoothing's host twins (uam_route3d_free_bits_host /
// uam_route3d_paths_smooth_host / uam_route3d_visible_host) for a sanitizer build: a hand-made
// volume with a terrain ridge, a blocked column and a blocked voxel, whose voxel count is no
// multiple of 32 (the bits buffer holds exactly uam_route3d_free_bits_bytes: a word read or
// written past it is seen), queried at every span class from inside, from outside the volume,
// by NaN, from a blocked voxel and with a bad goal index; sight lines across the whole volume,
// along its edges and through its corners.  CPU only; the device code is compiled as usual and
// never runs.
//   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Iinclude \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -o san_route3d_smooth tools/san_route3d_smooth.cpp \
//       uam_path_planning_amd/csrc/uampath.hip uam_path_planning_amd/csrc/polyproc.cpp \
//       uam_path_planning_amd/csrc/tiles.cpp -lz
//   ./san_route3d_smooth        (exit status 0 and "ok" on success)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "uampath.h"

namespace {

struct Volume {
    uam_volume_desc d;
    std::vector<uint32_t> words;  // exactly the voxels and the columns: a read past them is seen
    int64_t col_word;
    Volume(int nx, int ny, int nz) {
        d = {nx, ny, nz, 0.25, 3.0, 0.013, 0.0171, 40.0, 30.0};
        const int64_t col_off = ((int64_t)nx * ny * nz * 8 + 255) / 256 * 256;
        col_word = col_off / 4;
        words.assign((size_t)(col_word + (int64_t)nx * ny * 2), 0u);
    }
    void risk(int ix, int iy, int iz, float v) {
        std::memcpy(&words[(size_t)(((int64_t)iy * d.nx + ix) * d.nz + iz) * 2], &v, 4);
    }
    void column(int ix, int iy, float terrain, uint32_t flags) {
        const size_t i = (size_t)(col_word + ((int64_t)iy * d.nx + ix) * 2);
        std::memcpy(&words[i], &terrain, 4);
        words[i + 1] = flags;
    }
    void point(int ix, int iy, int iz, double* p) const {
        p[0] = d.x0 + (ix + 0.3) * d.dx;
        p[1] = d.y_top - (iy + 0.7) * d.dy;
        p[2] = d.z0 + (iz + 0.4) * d.dz;
    }
    int32_t index(int ix, int iy, int iz) const { return (iy * d.nx + ix) * d.nz + iz; }
};

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s (%s)\n", what, uam_last_error());
        ++failures;
    }
}

}  // namespace

int main() {
    const int NX = 21, NY = 13, NZ = 5;  // 1365 voxels: 42 full words and one of 21 bits
    Volume v(NX, NY, NZ);
    for (int iy = 0; iy < NY; ++iy)
        for (int ix = 0; ix < NX; ++ix) {
            for (int iz = 0; iz < NZ; ++iz) v.risk(ix, iy, iz, 0.5f);
            if (ix >= 9 && ix <= 10) v.column(ix, iy, 130.0f, 0u);  // layers 0..2 blocked
        }
    v.column(4, 4, 0.0f, UAM_FLAG_NFZ);
    v.risk(15, 6, 4, NAN);
    const uam_route3d_params p = {UAM_ABI_VERSION, 2.0, UAM_FLAG_NFZ, 1, 0, 10.0, 1e-3};
    const int64_t n = (int64_t)NX * NY * NZ;
    const int64_t bytes = uam_route3d_free_bits_bytes(&v.d);
    expect(bytes == (n + 31) / 32 * 4, "free_bits_bytes");
    std::vector<uint32_t> bits((size_t)(bytes / 4), 0xFFFFFFFFu);
    expect(uam_route3d_free_bits_host(&v.d, v.words.data(), &p, bits.data()) == UAM_OK,
           "free_bits_host");
    expect((bits.back() >> (n % 32)) == 0u, "the unused bits of the last word are 0");
    int64_t free_voxels = 0;
    for (uint32_t w : bits) free_voxels += __builtin_popcount(w);
    std::printf("%lld of %lld voxels free\n", (long long)free_voxels, (long long)n);
    expect(free_voxels > n / 2 && free_voxels < n, "free voxel count");

    const int32_t G = 2;
    std::vector<double> goals(6), dist((size_t)(G * n));
    std::vector<uint8_t> next((size_t)(G * n));
    v.point(18, 6, 0, &goals[0]);
    v.point(1, 11, 4, &goals[3]);
    expect(uam_route3d_field_host(&v.d, v.words.data(), &p, goals.data(), G, dist.data(),
                                  next.data()) == UAM_OK, "field_host");
    const int64_t Q = 9;
    std::vector<double> starts((size_t)(Q * 3));
    v.point(1, 6, 0, &starts[0]);                        // over the ridge
    v.point(0, 0, 4, &starts[3]);
    v.point(20, 12, 0, &starts[6]);
    v.point(18, 6, 0, &starts[9]);                       // in the goal voxel
    v.point(2, 2, 2, &starts[12]);
    starts[12] = v.d.x0 - 1e-3;                          // outside in x
    v.point(2, 2, 2, &starts[15]);
    starts[17] = NAN;                                    // by NaN
    v.point(4, 4, 1, &starts[18]);                       // in the blocked column
    v.point(9, 6, 1, &starts[21]);                       // inside the ridge
    v.point(1, 1, 1, &starts[24]);                       // a bad goal index
    const std::vector<int32_t> goal_idx = {0, 0, 1, 0, 0, 0, 0, 1, 2};
    const std::vector<int32_t> want = {0, 0, 0, 0, 1, 1, 1, 1, 4};
    const int32_t N = 9;
    std::vector<double> wp((size_t)(Q * (N + 2) * 3)), plain(wp.size());
    std::vector<int32_t> status((size_t)Q), steps((size_t)Q), vertices((size_t)Q), st0((size_t)Q),
        steps0((size_t)Q);
    expect(uam_route3d_paths_host(&v.d, v.words.data(), &p, next.data(), goals.data(), G,
                                  starts.data(), goal_idx.data(), Q, N, plain.data(), st0.data(),
                                  steps0.data()) == UAM_OK, "paths_host");
    for (int32_t span : {1, 2, 7, 64, 1024}) {
        expect(uam_route3d_paths_smooth_host(&v.d, &p, bits.data(), next.data(), goals.data(), G,
                                             starts.data(), goal_idx.data(), Q, N, span,
                                             wp.data(), status.data(), steps.data(),
                                             vertices.data()) == UAM_OK, "paths_smooth_host");
        std::printf("span %4d: vertices", span);
        for (int64_t q = 0; q < Q; ++q) {
            std::printf(" %d", vertices[(size_t)q]);
            expect(status[(size_t)q] == want[(size_t)q], "status");
            expect(steps[(size_t)q] == steps0[(size_t)q], "steps");
            expect((status[(size_t)q] == 0) == (vertices[(size_t)q] >= 2), "vertices");
        }
        std::printf("\n");
        if (span == 1)
            expect(std::memcmp(wp.data(), plain.data(), wp.size() * sizeof(double)) == 0,
                   "span 1 gives uam_route3d_paths_host's bits");
    }
    // steps and vertices may be NULL, and N = 0 leaves the two end points
    std::vector<double> ends((size_t)(Q * 6));
    expect(uam_route3d_paths_smooth_host(&v.d, &p, bits.data(), next.data(), goals.data(), G,
                                         starts.data(), goal_idx.data(), Q, 0, 64, ends.data(),
                                         status.data(), nullptr, nullptr) == UAM_OK,
           "paths_smooth_host N = 0");
    // sight lines: the volume's diagonals and edges in both directions, a voxel with itself,
    // the last voxel (the highest bit in use)
    const int32_t c000 = v.index(0, 0, 0), c111 = v.index(NX - 1, NY - 1, NZ - 1);
    const std::vector<int32_t> a = {c000, c111, v.index(NX - 1, 0, 0), v.index(0, NY - 1, NZ - 1),
                                    c000, c000, c000, c111, v.index(3, 3, 4), v.index(0, 0, 4)};
    const std::vector<int32_t> b = {c111, c000, v.index(0, NY - 1, NZ - 1), v.index(NX - 1, 0, 0),
                                    v.index(NX - 1, 0, 0), v.index(0, NY - 1, 0),
                                    v.index(0, 0, NZ - 1), c111, v.index(7, 7, 4),
                                    v.index(NX - 1, 0, 4)};
    std::vector<uint8_t> seen(a.size(), 7);
    expect(uam_route3d_visible_host(&v.d, bits.data(), (int64_t)a.size(), a.data(), b.data(),
                                    seen.data()) == UAM_OK, "visible_host");
    std::printf("visible:");
    for (uint8_t s : seen) {
        std::printf(" %d", s);
        expect(s <= 1, "visible_host writes 0 or 1");
    }
    std::printf("\n");
    expect(seen[0] == seen[1] && seen[2] == seen[3], "LOS3 is symmetric");
    expect(seen[5] == 1 && seen[6] == 1 && seen[7] == 1, "open edges and a voxel with itself");
    expect(seen[4] == 0 && seen[8] == 0, "the ridge and the blocked column hide");
    expect(seen[9] == 1, "above the ridge");
    const int32_t off = (int32_t)n;
    expect(uam_route3d_visible_host(&v.d, bits.data(), 1, &off, &c000, seen.data()) ==
               UAM_E_INVALID, "one index off the volume");
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
