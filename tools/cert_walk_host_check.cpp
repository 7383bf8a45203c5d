// Stand-alone host check of the sign certificate's list walk (trace_oct.hpp: ray_sign_certified / cert_walk against
// ray_sign_certified_ref), meant for a sanitizer build: it has its own main, loads nothing into an interpreter and needs no
// device.  For every non-empty list of two small tables -- the last list of the index area included, where a batch of the
// walk must not read a slot past the list's end as an index -- it sends rays into the list's cell and compares the batched
// walk (rtmi_debug_ray_cert_kappa) with the entry-at-a-time loop (rtmi_debug_ray_cert_ref), certificate and list length, at
// both bands.  Exit status 0: they agree everywhere.
//
// Build and run (from rust_raytrace_amd/csrc; host code with the sanitizers, device code as usual):
//   S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
//   for f in raytrace obj_parser capi; do hipcc -x c++ -O1 -g -std=c++17 -ffp-contract=off -fPIC $S -c host/$f.cpp -o /tmp/cw_$f.o; done
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fPIC -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -c device/rtmi_device.hip -o /tmp/cw_device.o
//   hipcc -x c++ -O1 -g -std=c++17 $S -c ../../tools/cert_walk_host_check.cpp -o /tmp/cw_main.o
//   hipcc --offload-arch=gfx950 $S /tmp/cw_*.o -pthread -o /tmp/cert_walk_host_check
//   ASAN_OPTIONS=detect_leaks=0 /tmp/cert_walk_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

extern "C" {
int rtmi_debug_ray_cert_kappa(const float* recs, uint64_t m, const float* rays, uint64_t n, uint32_t G, float kappa, uint8_t* cert,
                              uint32_t* ncand);
int rtmi_debug_ray_cert_ref(const float* recs, uint64_t m, const float* rays, uint64_t n, uint32_t G, float kappa, uint8_t* cert,
                            uint32_t* ncand);
int rtmi_debug_ray_cull(const float* recs, uint64_t m, const uint32_t* blocks, uint64_t nb, const float* rays, uint64_t n, uint32_t G,
                        uint32_t* packed, uint8_t* cert, uint32_t* ncand, uint32_t* cell, uint8_t* out, uint32_t* table, uint64_t table_cap,
                        uint64_t* table_words);
}

// records 1 .. n with the given (unnormalised) normals; record 0 is the sentinel
static std::vector<float> records(const std::vector<float>& nrm) {
    const size_t n = nrm.size() / 3;
    std::vector<float> r(8 * (n + 1), 0.f);
    for (size_t k = 0; k < n; k++) {
        float* p = &r[8 * (k + 1)];
        p[0] = 0.1f * (float)k; p[1] = -0.2f; p[2] = 0.3f; p[3] = 0.01f;
        p[4] = nrm[3 * k]; p[5] = nrm[3 * k + 1]; p[6] = nrm[3 * k + 2];
    }
    return r;
}

static int check(const char* what, const std::vector<float>& recs, uint32_t G) {
    const uint64_t m = recs.size() / 8;
    const float probe[8] = {0.f, 0.f, 0.f, 0.f, 1.f, 2.f, 3.f, 0.f};
    uint64_t words = 0;
    if (rtmi_debug_ray_cull(recs.data(), m, nullptr, 0, probe, 1, G, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &words)) return 1;
    std::vector<uint32_t> table(words);  // exactly the table's size: a read behind it is a heap overflow
    if (rtmi_debug_ray_cull(recs.data(), m, nullptr, 0, probe, 1, G, nullptr, nullptr, nullptr, nullptr, nullptr, table.data(), words, &words)) return 1;
    const uint32_t* off = &table[4];
    const size_t ncell = (size_t)3 * G * G;
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> in_cell(0.1f, 0.9f), scale(0.5f, 2.f);
    std::vector<float> rays;
    std::vector<uint32_t> want;
    size_t last = 0;
    for (size_t c = 0; c < ncell; c++) {
        if (off[c + 1] == off[c]) continue;
        last = c;
        const uint32_t face = (uint32_t)(c / ((size_t)G * G)), i = (uint32_t)((c / G) % G), j = (uint32_t)(c % G);
        for (int k = 0; k < 4; k++) {
            const float a = -1.f + 2.f * ((float)i + in_cell(rng)) / (float)G, b = -1.f + 2.f * ((float)j + in_cell(rng)) / (float)G, s = scale(rng);
            float d[3];
            d[face] = s; d[(face + 1) % 3] = a * s; d[(face + 2) % 3] = b * s;
            const float r[8] = {0.f, 0.f, 0.f, 0.f, d[0], d[1], d[2], 0.f};
            rays.insert(rays.end(), r, r + 8);
            want.push_back(off[c + 1] - off[c]);
        }
    }
    const uint64_t n = want.size();
    int bad = 0;
    size_t certified = 0, at_length = 0;
    for (float kappa : {1e-6f, 1e-9f}) {
        std::vector<uint8_t> c0(n), c1(n);
        std::vector<uint32_t> n0(n), n1(n);
        if (rtmi_debug_ray_cert_kappa(recs.data(), m, rays.data(), n, G, kappa, c0.data(), n0.data())) return 1;
        if (rtmi_debug_ray_cert_ref(recs.data(), m, rays.data(), n, G, kappa, c1.data(), n1.data())) return 1;
        for (uint64_t i = 0; i < n; i++) {
            if (c0[i] != c1[i] || n0[i] != n1[i]) {
                if (bad++ < 8) std::printf("%s kappa %g ray %llu: walk %u (%u listed), loop %u (%u listed)\n", what, kappa, (unsigned long long)i, c0[i], n0[i], c1[i], n1[i]);
            }
            certified += c0[i];
            at_length += n0[i] == want[i];  // (a ray on a cell's rim may round into the neighbour: reported, not required)
        }
    }
    std::printf("%s: G %u, %llu table words, %llu rays into %llu lists (the last one in cell %zu, %u entries, ends at %u of %u), "
                "%zu certified, %zu at the expected length, %d mismatches\n", what, G, (unsigned long long)words, (unsigned long long)n,
                (unsigned long long)(n / 4), last, off[last + 1] - off[last], off[last + 1], off[ncell], certified, at_length, bad);
    return bad != 0 || at_length == 0;
}

int main() {
    // five normals whose great circles pass through one cell of a G = 8 table (tests/test_ray_cert_walk_cpu.py, hand_scene)
    std::vector<float> hand;
    for (int j = 0; j < 5; j++) {
        const float a = (3 + 2 * j) / 128.f, b = (5 + 3 * j) / 128.f, p = 1.f + (float)(j % 3), q = 1.f + (float)(j / 3);
        hand.insert(hand.end(), {-(p * a + q * b), p, q});
    }
    // 300 random normals at G = 16: 768 lists of about 17 entries, whole batches and part-filled ones
    std::mt19937 rng(3);
    std::normal_distribution<float> g;
    std::vector<float> rnd;
    for (int k = 0; k < 900; k++) rnd.push_back(g(rng));
    int rc = check("hand-made", records(hand), 8);
    rc |= check("random", records(rnd), 16);
    std::printf(rc ? "FAILED\n" : "ok\n");
    return rc;
}
