// Stand-alone CPU sweep of the wide generator's host-side window arithmetic (csrc/ar_wide_plan.h): replays the loop of
// vqw_ar_wide_run_async over many (Tz, ratio, chunking) and checks that every step reads a frame its window holds, that a
// window never reaches past frame Tz - 1 and that the slot a kernel would index lies inside the buffer; then replays the
// prefill scatter (vqw_ar_wide_prefill_layer: the kept steps, their ring slots, the tiles of arw_prefill_scatter_kernel)
// over many (ring depth, prompt length, window, chunking) on bounds-checked buffers.  Build and run:
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

// The prefill scatter with the kernel's loop structure: grid (arw_tiles(nt), arw_tiles(nrows), R), a tile of rows x steps
// through a [32][33] buffer.  Every index goes through .at(); a tile element that is loaded must be stored and the other way
// round.  Returns the number of values stored, or -1.
static long long scatter(std::vector<float>& ring, int depth, int R, int B, const std::vector<float>& x, int ld, int t_first,
                         int t_end, int row0, int nrows) {
    const int t_lo = arw_prefill_first(t_end, depth), nt = arw_prefill_count(t_end, depth);
    long long stored = 0;
    for (int bz = 0; bz < R; ++bz)
        for (int by = 0; by < arw_tiles(nrows); ++by)
            for (int bx = 0; bx < arw_tiles(nt); ++bx) {
                std::vector<float> tile(AR_WIDE_PREFILL_TILE * (AR_WIDE_PREFILL_TILE + 1), -1.0f);
                std::vector<char> have(tile.size(), 0);
                const int s0 = bx * AR_WIDE_PREFILL_TILE, i0 = by * AR_WIDE_PREFILL_TILE;
                const int ns = arw_tile_extent(nt, bx), ni = arw_tile_extent(nrows, by);
                if (ns < 1 || ni < 1) return -1;                       // no empty tile is launched
                for (int tx = 0; tx < ns; ++tx)
                    for (int i = 0; i < ni; ++i) {
                        const size_t src = ((size_t)(i0 + i) * R + bz) * ld + (size_t)(t_lo - t_first + s0 + tx);
                        tile.at(i * (AR_WIDE_PREFILL_TILE + 1) + tx) = x.at(src);
                        have.at(i * (AR_WIDE_PREFILL_TILE + 1) + tx) = 1;
                    }
                for (int tx = 0; tx < ni; ++tx)
                    for (int sidx = 0; sidx < ns; ++sidx) {
                        if (!have.at(tx * (AR_WIDE_PREFILL_TILE + 1) + sidx)) return -1;
                        const int slot = arw_ring_slot(t_lo + s0 + sidx, depth);
                        ring.at(((size_t)slot * R + bz) * B + row0 + i0 + tx) = tile.at(tx * (AR_WIDE_PREFILL_TILE + 1) + sidx);
                        ++stored;
                    }
            }
    return stored;
}

#define PREQUIRE(c)                                                                                                     \
    do {                                                                                                                \
        if (!(c)) {                                                                                                     \
            std::printf("FAILED %s (line %d): depth %d t_end %d t_first %d ld %d B %d chunk %d\n", #c, __LINE__, depth, t_end, \
                        t_first, ld, B, chunk);                                                                         \
            return 1;                                                                                                   \
        }                                                                                                               \
    } while (0)

static int prefill_sweep(long long* values) {
    for (int it = 0; it < 4000; ++it) {
        const int depth = 1 + (int)rnd(it % 5 == 0 ? 100 : 34), R = 1 + (int)rnd(3), B = 1 + (int)rnd(it % 4 == 0 ? 130 : 40);
        const int t_end = (int)rnd((unsigned)(3 * depth + 2));
        const int t_lo = arw_prefill_first(t_end, depth), nt = arw_prefill_count(t_end, depth);
        const int t_first = (int)rnd((unsigned)(t_lo + 1)), ld = t_end - t_first + (int)rnd(5);
        int chunk = 1 + (int)rnd((unsigned)B);
        static const int around_a_tile[4] = {1, 7, 32, 33};
        if (it % 3 == 0) chunk = around_a_tile[rnd(4)];
        PREQUIRE(t_lo >= 0 && nt >= 0 && nt <= depth && t_lo + nt == t_end && (nt == depth || t_lo == 0));
        PREQUIRE(arw_prefill_covers(t_first, ld, t_end, depth));
        PREQUIRE(!arw_prefill_covers(t_lo + 1, ld, t_end, depth) && !arw_prefill_covers(-1, ld + 1, t_end, depth));
        PREQUIRE(t_end == t_first || !arw_prefill_covers(t_first, t_end - t_first - 1, t_end, depth));
        PREQUIRE(!arw_rows_inside(0, 0, B) && !arw_rows_inside(-1, 1, B) && !arw_rows_inside(B, 1, B) && !arw_rows_inside(1, B, B));
        PREQUIRE(arw_rows_inside(0, B, B) && arw_rows_inside(B - 1, 1, B) && !arw_rows_inside(1, 0x7fffffff, B));
        for (int tau = t_lo; tau < t_end; ++tau)            // the kept steps take distinct slots inside the ring
            for (int other = tau + 1; other < t_end; ++other) PREQUIRE(arw_ring_slot(tau, depth) != arw_ring_slot(other, depth));
        // x[b][r][c] encodes (b, r, step); the ring starts as reset leaves it
        const float UNTOUCHED = 0.0f;
        std::vector<float> ring((size_t)depth * R * B, UNTOUCHED);
        long long stored = 0;
        for (int row_hi = B; row_hi > 0; row_hi -= chunk) {   // chunks in descending row order, each with its own tensor
            const int row0 = row_hi - chunk > 0 ? row_hi - chunk : 0, nrows = row_hi - row0;
            PREQUIRE(arw_rows_inside(row0, nrows, B));
            PREQUIRE(arw_tiles(nrows) * AR_WIDE_PREFILL_TILE >= nrows && (arw_tiles(nrows) - 1) * AR_WIDE_PREFILL_TILE < nrows);
            std::vector<float> x((size_t)nrows * R * ld);
            for (int i = 0; i < nrows; ++i)
                for (int r = 0; r < R; ++r)
                    for (int c = 0; c < ld; ++c) x.at(((size_t)i * R + r) * ld + c) = 1.0f + (float)(((row0 + i) * 4 + r) * 512 + t_first + c);
            if (nt == 0) continue;                             // the call returns before it launches
            const long long n = scatter(ring, depth, R, B, x, ld, t_first, t_end, row0, nrows);
            PREQUIRE(n == (long long)nt * R * nrows);
            stored += n;
        }
        for (int slot = 0; slot < depth; ++slot)
            for (int r = 0; r < R; ++r)
                for (int b = 0; b < B; ++b) {
                    float want = UNTOUCHED;                    // a slot of a step before 0
                    for (int tau = t_lo; tau < t_end; ++tau)
                        if (tau % depth == slot) want = 1.0f + (float)((b * 4 + r) * 512 + tau);
                    PREQUIRE(ring.at(((size_t)slot * R + r) * B + b) == want);
                }
        *values += stored;
    }
    return 0;
}

int main() {
    long long values = 0;
    if (prefill_sweep(&values)) return 1;
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
    std::printf("ok: %lld steps, %lld window refreshes, %lld prefilled values\n", checked, refreshes, values);
    return 0;
}
