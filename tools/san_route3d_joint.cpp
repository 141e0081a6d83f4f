// Stand-alone driver of the volume's joint route field's host twins
// (uam_route3d_field_joint_host / uam_route3d_paths_joint_host, with uam_route3d_free_bits_host
// for the spans >= 1) for a sanitizer build.  It reads the cases
// tools/dump_route3d_joint_cases.py wrote (shared and invalid goals, the serpentine with chains
// of more than 1024 voxels, volumes of 1 x 1 x 1 and 3 x 2 x 2 voxels), runs the twins into
// buffers of exactly the documented sizes (a read or write past them is seen) and compares every
// output with the reference's bytes.  CPU only; the device code is compiled as usual and never
// runs.
//   python tools/dump_route3d_joint_cases.py joint3d_cases.bin
//   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Iinclude \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -o san_route3d_joint tools/san_route3d_joint.cpp \
//       uam_path_planning_amd/csrc/uampath.hip uam_path_planning_amd/csrc/polyproc.cpp \
//       uam_path_planning_amd/csrc/tiles.cpp -lz
//   ./san_route3d_joint joint3d_cases.bin       (exit status 0 and "ok" on success)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "uampath.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what, int32_t a = 0, int32_t b = 0) {
    if (!ok) {
        std::printf("FAILED: %s (case %d, span %d) (%s)\n", what, a, b, uam_last_error());
        ++failures;
    }
}

struct Reader {
    std::FILE* f;
    bool ok = true;
    template <typename T>
    std::vector<T> take(size_t n) {
        std::vector<T> v(n);
        if (n && std::fread(v.data(), sizeof(T), n, f) != n) ok = false;
        return v;
    }
    template <typename T>
    T one() {
        T v{};
        if (std::fread(&v, sizeof(T), 1, f) != 1) ok = false;
        return v;
    }
};

template <typename T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: %s CASES.bin\n", argv[0]);
        return 2;
    }
    Reader r{std::fopen(argv[1], "rb")};
    if (!r.f) {
        std::printf("cannot open %s\n", argv[1]);
        return 2;
    }
    const std::vector<char> magic = r.take<char>(8);
    if (!r.ok || std::memcmp(magic.data(), "UAMVJ001", 8)) {
        std::printf("%s is no case file\n", argv[1]);
        return 2;
    }
    const int32_t n_cases = r.one<int32_t>();
    for (int32_t ci = 0; ci < n_cases && r.ok; ++ci) {
        uam_volume_desc d{};
        d.nx = r.one<int32_t>(), d.ny = r.one<int32_t>(), d.nz = r.one<int32_t>();
        d.x0 = r.one<double>(), d.y_top = r.one<double>();
        d.dx = r.one<double>(), d.dy = r.one<double>();
        d.z0 = r.one<double>(), d.dz = r.one<double>();
        uam_route3d_params p{};
        p.abi_version = UAM_ABI_VERSION;
        p.lambda = r.one<double>();
        p.block_flags = r.one<uint32_t>();
        p.inflate = r.one<int32_t>();
        p.agl = r.one<double>();
        p.z_scale = r.one<double>();
        const int32_t G = r.one<int32_t>(), Q = r.one<int32_t>(), N = r.one<int32_t>(),
                      S = r.one<int32_t>(), W = r.one<int32_t>();
        if (!r.ok) break;
        const size_t n = (size_t)d.nx * d.ny * d.nz;
        // the voxels, then the columns at the 256-B aligned offset, and not a word more
        expect((size_t)W == (n * 8 + 255) / 256 * 64 + (size_t)d.nx * d.ny * 2, "volume words", ci);
        const auto vol = r.take<uint32_t>((size_t)W);
        const auto goals = r.take<double>((size_t)G * 3);
        const auto starts = r.take<double>((size_t)Q * 3);
        const auto dist_want = r.take<double>(n);
        const auto next_want = r.take<uint8_t>(n);
        const auto owner_want = r.take<int32_t>(n);
        if (!r.ok) break;
        std::vector<double> dist(n);
        std::vector<uint8_t> next(n);
        std::vector<int32_t> owner(n);
        expect(uam_route3d_field_joint_host(&d, vol.data(), &p, goals.data(), G, dist.data(),
                                            next.data(), owner.data()) == UAM_OK,
               "field_joint_host", ci);
        expect(same(dist, dist_want), "dist", ci);
        expect(same(next, next_want), "next", ci);
        expect(same(owner, owner_want), "owner", ci);
        const int64_t bytes = uam_route3d_free_bits_bytes(&d);
        expect(bytes == (int64_t)((n + 31) / 32) * 4, "free_bits_bytes", ci);
        std::vector<uint32_t> bits((size_t)(bytes / 4), 0xFFFFFFFFu);
        expect(uam_route3d_free_bits_host(&d, vol.data(), &p, bits.data()) == UAM_OK,
               "free_bits_host", ci);
        int32_t owned = 0;
        for (int32_t o : owner) owned += o >= 0;
        std::printf("case %d: %d x %d x %d voxels, %d goals, %d of %zu voxels owned\n", ci, d.nx,
                    d.ny, d.nz, G, owned, n);
        for (int32_t si = 0; si < S && r.ok; ++si) {
            const int32_t span = r.one<int32_t>();
            const auto wp_want = r.take<double>((size_t)Q * (N + 2) * 3);
            const auto status_want = r.take<int32_t>((size_t)Q);
            const auto steps_want = r.take<int32_t>((size_t)Q);
            const auto vertices_want = r.take<int32_t>((size_t)Q);
            const auto goal_want = r.take<int32_t>((size_t)Q);
            if (!r.ok) break;
            std::vector<double> wp(wp_want.size());
            std::vector<int32_t> status((size_t)Q), steps((size_t)Q), vertices((size_t)Q),
                goal((size_t)Q);
            // span 0 reads the volume and no bits, span >= 1 the bits and no volume
            expect(uam_route3d_paths_joint_host(&d, span ? nullptr : vol.data(), &p,
                                                span ? bits.data() : nullptr, next.data(),
                                                owner.data(), goals.data(), G, starts.data(), Q, N,
                                                span, wp.data(), status.data(), steps.data(),
                                                vertices.data(), goal.data()) == UAM_OK,
                   "paths_joint_host", ci, span);
            expect(same(wp, wp_want), "wp3", ci, span);
            expect(same(status, status_want), "status", ci, span);
            expect(same(steps, steps_want), "steps", ci, span);
            expect(same(vertices, vertices_want), "vertices", ci, span);
            expect(same(goal, goal_want), "goal", ci, span);
            // steps, vertices and goal_out may be NULL, and N = 0 leaves the two end points
            std::vector<double> ends((size_t)Q * 6);
            expect(uam_route3d_paths_joint_host(&d, vol.data(), &p, bits.data(), next.data(),
                                                owner.data(), goals.data(), G, starts.data(), Q, 0,
                                                span, ends.data(), status.data(), nullptr, nullptr,
                                                nullptr) == UAM_OK,
                   "paths_joint_host N = 0", ci, span);
            expect(same(status, status_want), "status N = 0", ci, span);
        }
    }
    expect(r.ok, "the case file is complete");
    std::fclose(r.f);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
