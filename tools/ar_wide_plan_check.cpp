// Stand-alone CPU sweep of the wide generator's host-side window arithmetic (csrc/ar_wide_plan.h): replays the loop of
// vqw_ar_wide_run_async over many (Tz, ratio, chunking) and checks that every step reads a frame its window holds, that a
// window never reaches past frame Tz - 1 and that the slot a kernel would index lies inside the buffer.  Build and run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ar_wide_plan_check.cpp -o ar_wide_plan_check && ./ar_wide_plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../vq-vae-wavenet_amd/csrc/ar_wide_plan.h"

static unsigned long long rng = 88172645463325252ull;
static unsigned rnd(unsigned n) {
    rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
    return (unsigned)(rng % n);
}

#define REQUIRE(c)                                                                        \
    do {                                                                                  \
        if (!(c)) { std::printf("FAILED %s (line %d): Tz %d ratio %d t %lld\n", #c, __LINE__, Tz, ratio, t); return 1; } \
    } while (0)

int main() {
    long long checked = 0, refreshes = 0;
    for (int it = 0; it < 20000; ++it) {
        const int Tz = 1 + (int)rnd(it % 7 == 0 ? 40 : 12), ratio = 1 + (int)rnd(it % 3 == 0 ? 70 : 5);
        const long long total = 1 + rnd((unsigned)(Tz * ratio * 2));   // also past the last frame
        long long t = 0;
        std::vector<int> condwin(AR_WIDE_WINDOW, -1);   // the frame each slot holds
        while (t < total) {
            long long left = 1 + rnd((unsigned)(total - t));   // one run (chunk): its windows start afresh
            ArWideWindow win;
            while (left > 0) {
                const int frame = arw_frame(t, ratio, Tz);
                REQUIRE(frame >= 0 && frame < Tz);
                if (!arw_window_holds(win, frame)) {
                    win = arw_window_at(frame, Tz);
                    REQUIRE(win.nf >= 1 && win.nf <= AR_WIDE_WINDOW && win.f0 + win.nf <= Tz);
                    for (int f = 0; f < win.nf; ++f) condwin.at(f) = win.f0 + f;
                    ++refreshes;
                }
                const long long n = arw_steps_in_window(win, t, left, ratio, Tz);
                REQUIRE(n >= 1 && n <= left);
                for (long long i = 0; i < n; ++i) {   // what the kernels index
                    const int f = arw_frame(t + i, ratio, Tz) - win.f0;
                    REQUIRE(f >= 0 && f < win.nf);
                    REQUIRE(condwin.at(f) == arw_frame(t + i, ratio, Tz));
                    ++checked;
                }
                t += n;
                left -= n;
            }
        }
    }
    std::printf("ok: %lld steps, %lld window refreshes\n", checked, refreshes);
    return 0;
}
