// Host-side index arithmetic of the wide generator (ar_wide.hip): which condition frame a step reads, when the window of
// projected condition frames has to be refreshed and what it then covers.  Plain C++ with no HIP in it, so a stand-alone
// program can sweep it on the CPU (tools/ar_wide_plan_check.cpp).
#pragma once

constexpr int AR_WIDE_WINDOW = 4;   // condition frames projected at a time

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
