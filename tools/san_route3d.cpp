// Stand-alone driver of the volume route seeds' host twins (uam_route3d_field_host /
// uam_route3d_paths_host) for a sanitizer build: two hand-made volumes -- an open one with a
// blocked column, and a terrain ridge with inflation and a clearance -- queried from inside,
// from outside the volume in x and in z, by NaN, from a blocked voxel and with bad goal indices.
// CPU only; the device code is compiled as usual and never runs.
//   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Iinclude \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -o san_route3d tools/san_route3d.cpp uam_path_planning_amd/csrc/uampath.hip \
//       uam_path_planning_amd/csrc/polyproc.cpp uam_path_planning_amd/csrc/tiles.cpp -lz
//   ./san_route3d        (exit status 0 and "ok" on success)
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
};

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s (%s)\n", what, uam_last_error());
        ++failures;
    }
}

void run(const char* name, const Volume& v, const uam_route3d_params& p,
         const std::vector<double>& goals, const std::vector<double>& starts,
         const std::vector<int32_t>& goal_idx, const std::vector<int32_t>& want, int32_t N) {
    const int32_t G = (int32_t)(goals.size() / 3);
    const int64_t Q = (int64_t)goal_idx.size();
    const int64_t n = (int64_t)v.d.nx * v.d.ny * v.d.nz;
    std::vector<double> dist((size_t)(G * n));
    std::vector<uint8_t> next((size_t)(G * n));
    expect(uam_route3d_field_host(&v.d, v.words.data(), &p, goals.data(), G, dist.data(),
                                  next.data()) == UAM_OK, "field_host");
    std::vector<double> wp((size_t)(Q * (N + 2) * 3));
    std::vector<int32_t> status((size_t)Q), steps((size_t)Q);
    expect(uam_route3d_paths_host(&v.d, v.words.data(), &p, next.data(), goals.data(), G,
                                  starts.data(), goal_idx.data(), Q, N, wp.data(), status.data(),
                                  steps.data()) == UAM_OK, "paths_host");
    int64_t finite = 0;
    for (double x : dist) finite += std::isfinite(x) ? 1 : 0;
    std::printf("%s: %lld finite voxels; status", name, (long long)finite);
    for (int64_t q = 0; q < Q; ++q) {
        std::printf(" %d", status[(size_t)q]);
        expect(status[(size_t)q] == want[(size_t)q], "status");
        expect((status[(size_t)q] == 0) == (steps[(size_t)q] > 0), "steps");
    }
    std::printf("\n");
    // steps may be NULL, and N = 0 leaves the two end points
    std::vector<double> ends((size_t)(Q * 6));
    expect(uam_route3d_paths_host(&v.d, v.words.data(), &p, next.data(), goals.data(), G,
                                  starts.data(), goal_idx.data(), Q, 0, ends.data(),
                                  status.data(), nullptr) == UAM_OK, "paths_host N = 0");
}

}  // namespace

int main() {
    const int NX = 21, NY = 13, NZ = 6;
    {
        Volume v(NX, NY, NZ);
        for (int iy = 0; iy < NY; ++iy)
            for (int ix = 0; ix < NX; ++ix)
                for (int iz = 0; iz < NZ; ++iz)
                    v.risk(ix, iy, iz, 0.125f * (float)((ix * 7 + iy * 3 + iz * 5) % 11));
        v.column(4, 4, 0.0f, UAM_FLAG_NFZ);
        v.risk(9, 9, 2, NAN);
        const uam_route3d_params p = {UAM_ABI_VERSION, 1.0, UAM_FLAG_NFZ, 0, 0, 0.0, 1e-3};
        std::vector<double> goals(6), starts(8 * 3);
        v.point(15, 6, 3, &goals[0]);
        goals[3] = 99.0, goals[4] = 99.0, goals[5] = 100.0;   // outside the volume
        v.point(15, 6, 3, &starts[0]);                        // in the goal voxel
        v.point(0, 0, 0, &starts[3]);
        v.point(NX - 1, NY - 1, NZ - 1, &starts[6]);
        v.point(2, 2, 2, &starts[9]);
        starts[9] = v.d.x0 - 1e-3;                            // outside in x
        v.point(2, 2, 2, &starts[12]);
        starts[14] = v.d.z0 + NZ * v.d.dz + 1.0;              // outside in z
        v.point(2, 2, 2, &starts[15]);
        starts[16] = NAN;                                     // by NaN
        v.point(4, 4, 1, &starts[18]);                        // in the blocked column
        v.point(1, 1, 1, &starts[21]);
        run("open", v, p, goals, starts, {0, 0, 0, 0, 0, 0, 0, 1}, {0, 0, 0, 1, 1, 1, 1, 4}, 9);
    }
    {
        Volume v(NX, NY, NZ);
        for (int iy = 0; iy < NY; ++iy)
            for (int ix = 0; ix < NX; ++ix) {
                for (int iz = 0; iz < NZ; ++iz) v.risk(ix, iy, iz, 0.5f);
                if (ix >= 9 && ix <= 11) v.column(ix, iy, 130.0f, 0u);   // layers 0..2 blocked
            }
        const uam_route3d_params p = {UAM_ABI_VERSION, 4.0, UAM_FLAG_NFZ, 2, 0, 10.0, 1e-3};
        std::vector<double> goals(3), starts(5 * 3);
        v.point(18, 6, 0, &goals[0]);
        v.point(1, 6, 0, &starts[0]);
        v.point(0, 0, 5, &starts[3]);
        v.point(10, 6, 5, &starts[6]);                        // above the ridge
        v.point(10, 6, 1, &starts[9]);                        // inside it
        v.point(7, 6, 1, &starts[12]);                        // within the inflation
        run("ridge", v, p, goals, starts, {0, 0, 0, 0, -1}, {0, 0, 0, 1, 4}, 9);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
