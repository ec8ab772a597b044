// Host-only check of the directional round loop (rogtk_amd/csrc/directional_rounds.h) against
// a model of the relaxation kernel, for the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -I rogtk_amd/csrc tools/directional_rounds_check.cpp \
//       -o /tmp/directional_rounds_check && /tmp/directional_rounds_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "directional_rounds.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED %s (line %d)\n", #cond, __LINE__);   \
            ++failures;                                               \
        }                                                             \
    } while (0)

// A path v0 -> v1 -> ... -> v(m-1) relaxed against the order of the lanes (descending v), so
// that one round moves the best key one edge only: the slowest case the cap allows.
struct PathModel {
    std::vector<int64_t> best;
    std::vector<uint32_t> words;
    int64_t launched = 0;
    explicit PathModel(int64_t m) : best((size_t)m), words(rogtk::kDirBatch, 0u) {
        for (int64_t v = 0; v < m; ++v) best[(size_t)v] = m - v;  // v0 holds the largest key
    }
    int launch(int64_t first, int k) {
        if (first != launched) return 99;
        for (auto& w : words) w = 0;
        for (int j = 0; j < k; ++j) {
            for (int64_t v = (int64_t)best.size() - 1; v >= 1; --v) {
                if (best[(size_t)v - 1] > best[(size_t)v]) {
                    best[(size_t)v] = best[(size_t)v - 1];
                    words[(size_t)j] = 1;
                }
            }
            ++launched;
        }
        return 0;
    }
    int read(int k, uint32_t* changed) const {
        for (int j = 0; j < k; ++j) changed[j] = words[(size_t)j];
        return 0;
    }
};

void path(int64_t m, int64_t want_rounds) {
    PathModel g(m);
    int64_t rounds = -1;
    const int rc = rogtk::directional_run_rounds(
        m, [&](int64_t f, int k) { return g.launch(f, k); }, [&](int k, uint32_t* c) { return g.read(k, c); }, &rounds);
    EXPECT(rc == 0);
    EXPECT(rounds == want_rounds);
    EXPECT(g.launched <= (m > 1 ? m : 1));
    for (int64_t v = 0; v < m; ++v) EXPECT(g.best[(size_t)v] == m);
}

}  // namespace

int main() {
    for (int64_t m : {1, 2, 3, 4, 5, 7, 8, 9, 300}) path(m, m);  // m - 1 rounds move, round m confirms
    {
        int64_t rounds = -1, launched = 0;  // a kernel that never settles: an error at the cap
        const int rc = rogtk::directional_run_rounds(
            10,
            [&](int64_t, int k) {
                launched += k;
                return 0;
            },
            [&](int k, uint32_t* c) {
                for (int j = 0; j < k; ++j) c[j] = 1;
                return 0;
            },
            &rounds);
        EXPECT(rc == -1 && rounds == 10 && launched == 10);
    }
    {
        int64_t rounds = -1;  // errors of the two callbacks come back as they are
        EXPECT(rogtk::directional_run_rounds(5, [](int64_t, int) { return 2; }, [](int, uint32_t*) { return 0; },
                                             &rounds) == 2);
        EXPECT(rogtk::directional_run_rounds(5, [](int64_t, int) { return 0; }, [](int, uint32_t*) { return 3; },
                                             &rounds) == 3);
    }
    {
        int64_t rounds = -1;  // no vertices: one round that changes nothing
        EXPECT(rogtk::directional_run_rounds(0, [](int64_t, int) { return 0; }, [](int, uint32_t*) { return 0; },
                                             &rounds) == 0 && rounds == 1);
    }
    std::printf(failures ? "directional_rounds_check: %d failures\n" : "directional_rounds_check: ok\n", failures);
    return failures ? 1 : 0;
}
