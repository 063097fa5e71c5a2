// LDS image of the weight gradients' plane operands when both arrive by LDS-DMA (f16x3_wgrad.hip): the layout as
// constexpr functions that the kernel uses and that are checked below at compile time -- no GPU needed.
//
// An operand plane of one 16-step stage is [16 time steps][256 channels] of 16-bit pieces = 32 chunks of 16 bytes per step.  An
// LDS-DMA writes a lane-linear 1-KiB piece (lane i at + 16 i), so a piece is 8 time steps x 8 chunks, lane = 8 step + slot: a row
// (one time step) is 128 bytes and a stage holds 2 (time halves) x 4 (groups of 8 chunks = 64 channels) pieces per plane.  With
// plain rows the four rows of a transposed read (ds_read_b64_tr_b16: 4 time steps x 16 channels = 4 x 32 bytes per 16 lanes) would
// start 128 bytes apart: two of them on the same banks.  So the lane for (step, slot) FETCHES chunk slot ^ 4 ((step >> 1) & 1) of
// its group -- the permutation is on the source side, the destination stays lane-linear -- and the read applies the same XOR:
// rows q = 0..3 of a 32-lane half then start at 0 / 128 / 64 / 192 (mod 256) or at 64 / 192 / 0 / 128, four different 64-byte
// bank groups.
#pragma once

namespace wgl {

constexpr int PIECE = 1024;                 // bytes one LDS-DMA instruction of a wave writes
constexpr int STEPS = 8, SLOTS = 8;         // time steps x 16-byte chunks of a piece
constexpr int PLANE = 8 * PIECE;            // a plane of a stage: pieces [time half][chunk group]

// which chunk of its 8-chunk group the lane for (step, slot) fetches, and in which slot of row `step` chunk c is found
constexpr int swz(int step, int c) { return c ^ (4 * ((step >> 1) & 1)); }
// byte offset of piece (plane, time half, chunk group) in an operand's image of a stage
constexpr int piece_off(int plane, int thalf, int cgroup) { return ((plane * 2 + thalf) * 4 + cgroup) * PIECE; }
// byte offset of (time step t of the stage's 16, chunk c of the plane's 32) in a plane of the image
constexpr int entry_off(int t, int c) { return piece_off(0, t >> 3, c >> 3) + (t & 7) * (SLOTS * 16) + swz(t & 7, c & 7) * 16; }

// Transposed fragment read of a 32-channel tile (row tile i of p, column tile of q): the lane's address inside its plane's image.
// 16-lane group G = lane / 16 reads time steps 8 (G / 2) + 4 khalf + 0..3 and 16 channels from 16 (G % 2) of the tile; its lane
// 4 q + p supplies the address of row q, channels 4 p .. 4 p + 3, and receives channel lane % 16 with row q in element q.
constexpr int tr_addr(int lane, int tile, int khalf) {
    const int t = 8 * (lane >> 5) + 4 * khalf + ((lane & 15) >> 2);
    const int ch = 32 * tile + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    return entry_off(t, ch >> 3) + (ch & 7) * 2;
}
// The kernel forms tr_addr from one lane term, an XOR for odd tiles and constants:
constexpr int tr_lane(int lane) { return tr_addr(lane, 0, 0); }
constexpr int tr_addr_split(int lane, int tile, int khalf) {
    return piece_off(0, 0, tile >> 1) + (tr_lane(lane) ^ ((tile & 1) * 64)) + khalf * 4 * (SLOTS * 16);
}

// 2 x 2 wave tiling of the 256 x 256 output tile: wave (wr, wc) = (wave >> 1, wave & 1) owns rows 128 wr .. and columns 128 wc ..,
// i.e. row tiles 4 wr + i of p and column tiles 4 wc + j of q (i, j = 0..3): 8 A + 8 B fragments per step instead of 16 + 4.
constexpr int WAVES = 4, WTILES = 4;
constexpr int wave_a_tile(int wave, int i) { return WTILES * (wave >> 1) + i; }
constexpr int wave_b_tile(int wave, int j) { return WTILES * (wave & 1) + j; }
// the q sums of a column tile are formed by one of the two waves that read it: wave (wr, wc) sums j = 2 wr + h (h = 0, 1) of its four
constexpr int wave_sum_j(int wave, int h) { return 2 * (wave >> 1) + h; }
// The kernel forms a fragment's address from a wave term (per operand), the lane term, an XOR for odd tiles and constants:
constexpr int wave_a_off(int wave) { return piece_off(0, 0, 2 * (wave >> 1)); }
constexpr int wave_b_off(int wave) { return piece_off(0, 0, 2 * (wave & 1)); }
constexpr int wave_addr_split(int wave_off, int lane, int k, int khalf) {      // k: the wave's own tile index i or j
    return wave_off + piece_off(0, 0, k >> 1) + (tr_lane(lane) ^ ((k & 1) * 64)) + khalf * 4 * (SLOTS * 16);
}

// ---- compile-time checks
// what the DMA puts at byte `a` of a plane's image: (time step of the stage) * 256 + channel
constexpr int dma_content(int a) {
    const int piece = a / PIECE, lane = (a % PIECE) / 16, step = lane >> 3, slot = lane & 7;
    const int thalf = piece >> 2, cgroup = piece & 3;
    const int chunk = cgroup * 8 + swz(step, slot);
    return (thalf * 8 + step) * 256 + chunk * 8 + (a % 16) / 2;
}
// (a) source map and read map are the same involution, and the read finds every entry where the lane-linear write put it
constexpr bool check_involution() {
    for (int step = 0; step < STEPS; ++step)
        for (int c = 0; c < SLOTS; ++c) {
            if (swz(step, swz(step, c)) != c) return false;
            // the lane that fetched chunk c is lane 8 step + swz(step, c): it lands at 16 * lane, where entry_off looks for (step, c)
            if (entry_off(step, c) != (8 * step + swz(step, c)) * 16) return false;
        }
    for (int t = 0; t < 16; ++t)
        for (int c = 0; c < 32; ++c)
            if (dma_content(entry_off(t, c)) != t * 256 + c * 8) return false;
    return true;
}
// (b) every fragment element of every tile and k half is its (channel, time step): lane (channel n = lane % 32, k half lane / 32)
// of the MFMA operand holds time steps 8 (lane / 32) + 0..7 of channel 32 tile + n
constexpr bool check_fragments() {
    for (int tile = 0; tile < 8; ++tile)
        for (int kh = 0; kh < 2; ++kh)
            for (int lane = 0; lane < 64; ++lane) {
                if (tr_addr_split(lane, tile, kh) != tr_addr(lane, tile, kh)) return false;
                if (tr_addr(lane, tile, kh) % 8 != 0) return false;
                for (int q = 0; q < 4; ++q) {
                    // element q of the lane comes from the row addressed by lane 4 q + (lane % 16) / 4 of its group, column lane % 4
                    const int src = (lane & ~15) + 4 * q + ((lane & 15) >> 2);
                    const int a = tr_addr(src, tile, kh) + 2 * (lane & 3);
                    const int want_t = 8 * (lane >> 5) + 4 * kh + q, want_ch = 32 * tile + (lane & 31);
                    if (dma_content(a) != want_t * 256 + want_ch) return false;
                }
            }
    return true;
}
// (c) bank rule of ds_read_b64_tr_b16: bank (a / 4) % 64, conflicts per 32-lane half.  The four rows of a half lie in four different
// 64-byte bank groups, and no two lanes of a half share a bank.
constexpr bool check_banks() {
    for (int tile = 0; tile < 8; ++tile)
        for (int kh = 0; kh < 2; ++kh)
            for (int half = 0; half < 2; ++half) {
                bool used[64] = {};
                int group_of_row[4] = {-1, -1, -1, -1};
                for (int l = 0; l < 32; ++l) {
                    const int lane = 32 * half + l, a = tr_addr(lane, tile, kh), q = (lane & 15) >> 2;
                    const int grp = (a / 64) % 4;
                    if (group_of_row[q] >= 0 && group_of_row[q] != grp) return false;
                    group_of_row[q] = grp;
                    for (int w = 0; w < 2; ++w) {
                        const int bank = (a / 4 + w) % 64;
                        if (used[bank]) return false;
                        used[bank] = true;
                    }
                }
                for (int q = 0; q < 4; ++q)
                    for (int r = 0; r < q; ++r)
                        if (group_of_row[q] == group_of_row[r]) return false;
            }
    return true;
}
// (d) the 2 x 2 wave tiling: the kernel's address of every (wave, own tile, k half) is the checked read map (b, c) at the tile the
// wave owns -- so every fragment element is its (channel, time step) and no two lanes of a half share a bank, in every plane (a
// plane is an offset of PLANE: the same banks) --, the 4 x 16 (row tile, column tile) pairs of the waves are the tile's 64, each
// once, and every column tile is summed by exactly one wave, from a fragment that wave reads.
constexpr bool check_wave_tiling() {
    int owners[8][8] = {}, summed[8] = {};
    for (int wave = 0; wave < WAVES; ++wave) {
        for (int k = 0; k < WTILES; ++k)
            for (int kh = 0; kh < 2; ++kh)
                for (int lane = 0; lane < 64; ++lane) {
                    if (wave_addr_split(wave_a_off(wave), lane, k, kh) != tr_addr(lane, wave_a_tile(wave, k), kh)) return false;
                    if (wave_addr_split(wave_b_off(wave), lane, k, kh) != tr_addr(lane, wave_b_tile(wave, k), kh)) return false;
                    for (int q = 0; q < 4; ++q) {
                        const int src = (lane & ~15) + 4 * q + ((lane & 15) >> 2);
                        const int want_t = 8 * (lane >> 5) + 4 * kh + q;
                        if (dma_content(wave_addr_split(wave_a_off(wave), src, k, kh) + 2 * (lane & 3)) != want_t * 256 + 32 * wave_a_tile(wave, k) + (lane & 31)) return false;
                        if (dma_content(wave_addr_split(wave_b_off(wave), src, k, kh) + 2 * (lane & 3)) != want_t * 256 + 32 * wave_b_tile(wave, k) + (lane & 31)) return false;
                    }
                }
        for (int i = 0; i < WTILES; ++i)
            for (int j = 0; j < WTILES; ++j) {
                if (wave_a_tile(wave, i) < 0 || wave_a_tile(wave, i) >= 8 || wave_b_tile(wave, j) < 0 || wave_b_tile(wave, j) >= 8) return false;
                ++owners[wave_a_tile(wave, i)][wave_b_tile(wave, j)];
            }
        for (int h = 0; h < 2; ++h) {
            if (wave_sum_j(wave, h) < 0 || wave_sum_j(wave, h) >= WTILES) return false;
            ++summed[wave_b_tile(wave, wave_sum_j(wave, h))];
        }
    }
    for (int i = 0; i < 8; ++i) {
        if (summed[i] != 1) return false;
        for (int j = 0; j < 8; ++j)
            if (owners[i][j] != 1) return false;
    }
    return true;
}
static_assert(check_involution(), "wgrad LDS image: source permutation and read permutation differ");
static_assert(check_wave_tiling(), "wgrad LDS image: the 2 x 2 wave tiling reads a fragment that is not its tile's, or leaves a tile out");
static_assert(check_fragments(), "wgrad LDS image: a fragment element is not its (channel, time step)");
static_assert(check_banks(), "wgrad LDS image: bank conflict in a transposed read");

}  // namespace wgl
