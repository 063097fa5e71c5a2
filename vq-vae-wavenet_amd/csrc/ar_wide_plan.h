// Host-side index arithmetic of the wide generator (ar_wide.hip): which condition frame a step reads, when the window of
// projected condition frames has to be refreshed and what it then covers, and the ranges, slots and tiles of a prefill.
// Plain C++ with no HIP in it, so a stand-alone program can sweep it on the CPU (tools/ar_wide_plan_check.cpp).
#pragma once

constexpr int AR_WIDE_WINDOW = 4;   // condition frames projected at a time

constexpr int AR_WIDE_PREFILL_TILE = 32;   // rows and steps of one tile of the prefill scatter (arw_prefill_scatter_kernel)

// ---- prefill (vqw_ar_wide_prefill_layer): which steps of a prompt of t_end steps a ring of `depth` slots keeps, where each
// goes, and how a range of n rows or steps is cut into tiles.  constexpr: the scatter kernel calls the same functions.
// the first step the ring keeps: steps [first, t_end) are the last `depth` ones, none before step 0
constexpr int arw_prefill_first(int t_end, int depth) { return t_end > depth ? t_end - depth : 0; }

// how many it keeps: min(t_end, depth)
constexpr int arw_prefill_count(int t_end, int depth) { return t_end - arw_prefill_first(t_end, depth); }

// the ring slot of step tau >= 0: the one the layer's output kernel pushes it to (step % ring_depth)
constexpr int arw_ring_slot(int tau, int depth) { return tau % depth; }

// columns [t_first, t_first + ld) of the caller's tensor hold steps [arw_prefill_first, t_end)
constexpr bool arw_prefill_covers(int t_first, int ld, int t_end, int depth) {
    return t_first >= 0 && t_first <= arw_prefill_first(t_end, depth) && (long long)t_first + ld >= t_end;
}

// rows [row0, row0 + nrows) lie inside a handle of B rows
constexpr bool arw_rows_inside(int row0, int nrows, int B) { return nrows >= 1 && row0 >= 0 && row0 <= B - nrows; }

// tiles of AR_WIDE_PREFILL_TILE that cover n items, and how many items tile i holds (the last one may be partial)
constexpr int arw_tiles(int n) { return (n + AR_WIDE_PREFILL_TILE - 1) / AR_WIDE_PREFILL_TILE; }
constexpr int arw_tile_extent(int n, int i) {
    return n - i * AR_WIDE_PREFILL_TILE >= AR_WIDE_PREFILL_TILE ? AR_WIDE_PREFILL_TILE
           : n - i * AR_WIDE_PREFILL_TILE > 0                   ? n - i * AR_WIDE_PREFILL_TILE
                                                                : 0;
}

// the condition frame of step t: a step past the last frame keeps frame Tz - 1
inline int arw_frame(long long t, int ratio, int Tz) {
    const long long f = t / ratio;
    return f >= Tz ? Tz - 1 : (int)f;
}

struct ArWideWindow {
    int f0 = 0, nf = 0;   // frames [f0, f0 + nf) are projected; nf = 0: nothing is
};

inline bool arw_window_holds(const ArWideWindow& w, int frame) { return frame >= w.f0 && frame < w.f0 + w.nf; }

// the window that starts at `frame`: at most AR_WIDE_WINDOW frames, none past Tz - 1
inline ArWideWindow arw_window_at(int frame, int Tz) {
    ArWideWindow w;
    w.f0 = frame;
    w.nf = Tz - frame < AR_WIDE_WINDOW ? Tz - frame : AR_WIDE_WINDOW;
    return w;
}

// steps from t on (at most n) that the window still serves: up to the first step whose frame lies past it
inline long long arw_steps_in_window(const ArWideWindow& w, long long t, long long n, int ratio, int Tz) {
    if (w.f0 + w.nf >= Tz) return n;                       // holds frame Tz - 1, which every later step reads
    const long long end = (long long)(w.f0 + w.nf) * ratio;   // first step of the frame behind the window
    return end - t < n ? end - t : n;
}
