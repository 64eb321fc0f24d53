// Grid planner of the mixed-tile conv launch (conv1d_mfma_mixed_kernel in rca_codec.hip).  Plain C++, no HIP: the host tests compile
// this header alone.
//
// Every wave of a conv launch is its own workgroup and all waves of a launch are the same size, so a launch of W waves on a chip that
// holds `simds * occ` of them ends on a part-filled round: the chip is busy for ceil(W / simds) waves per SIMD where the work is only
// W / simds.  The plan keeps the bulk wave tile for the whole rounds and cuts the columns that are left into finer tiles placed at the
// end of the grid (largest jobs first): slots that free up while the bulk drains pick them up and the SIMDs finish together.
// A wave tile changes no arithmetic (every output is one fma chain in the same order), so any plan gives the same bits.
#pragma once

struct ConvBalancePlan {
    long bulk_col_tiles;     // column tiles of the bulk shape, a multiple of 8; the columns from bulk_col_tiles * bulk_wn * 32 on are fine
    int fine_wm, fine_wn;    // fine wave tile in units of 32 channels x 32 columns; 0 x 0: no remainder, launch the single-shape grid
    long finish;             // modelled finish: MFMAs (per k pair) issued by the most loaded SIMD, waves dealt evenly
    long finish_single;      // the same for the single-shape grid
};

static inline long conv_balance_cdiv(long a, long b) { return (a + b - 1) / b; }

// modelled finish of `bulk` column tiles of wm x wn waves followed by the rest of `total` column tiles as fwm x fwn waves
static inline long conv_balance_finish(long total, long bulk, int n_co_bulk, int simds, int wm, int wn, int fwm, int fwn) {
    const long bulk_waves = bulk * n_co_bulk;
    const long fine_waves = (total - bulk) * (wn / fwn) * n_co_bulk * (wm / fwm);
    return conv_balance_cdiv(bulk_waves, simds) * (wm * wn) + conv_balance_cdiv(fine_waves, simds) * (fwm * fwn);
}

// total_col_tiles: column tiles of the bulk shape that hold a column (not padded); n_co_bulk: channel tiles of the bulk shape;
// simds: 4 x compute units; occ_bulk: resident waves per SIMD of the bulk instantiation; (wm, wn): bulk wave tile in units of 32.
// The bulk is the largest whole number of rounds (simds * occ_bulk waves), rounded down to 8 column tiles (one per XCD); one round
// fewer is tried as well, with 32 x 64 and 32 x 32 remainders, and the smallest modelled finish wins -- ties keep the larger bulk and
// the larger fine tile (fewer waves, fewer fetches).  Under one round, without a remainder, or when no candidate models below the
// single-shape grid, the plan is that grid.
static inline ConvBalancePlan conv_balance_plan(long total_col_tiles, int n_co_bulk, int simds, int occ_bulk, int wm, int wn) {
    ConvBalancePlan p{total_col_tiles, 0, 0, 0, 0};
    if (total_col_tiles <= 0 || n_co_bulk <= 0 || simds <= 0 || occ_bulk <= 0) return p;
    const long waves = total_col_tiles * n_co_bulk, round = (long)simds * occ_bulk;
    p.finish = p.finish_single = conv_balance_cdiv(waves, simds) * (wm * wn);
    if (waves < round) return p;
    const long rounds = waves / round;
    static const int fine[2][2] = {{1, 2}, {1, 1}};
    for (long r = rounds; r >= 1 && r + 1 >= rounds; --r) {
        long bulk = (r * round / n_co_bulk) / 8 * 8;
        if (bulk > total_col_tiles) bulk = total_col_tiles / 8 * 8;
        if (bulk <= 0 || bulk >= total_col_tiles) continue;
        for (const auto& f : fine) {
            if (f[0] > wm || f[1] > wn || f[0] * f[1] >= wm * wn) continue;
            const long fin = conv_balance_finish(total_col_tiles, bulk, n_co_bulk, simds, wm, wn, f[0], f[1]);
            if (fin < p.finish) p = ConvBalancePlan{bulk, f[0], f[1], fin, p.finish_single};
        }
    }
    return p;
}

// RCA_CONV_BALANCE_PLAN=<bulk_col_tiles>:<32x64|32x32> (tests): the seam where the text says, rounded down to 8 column tiles and clamped to
// the launch.  false: the text is not a plan, or names a fine tile that is not finer than the bulk tile.
static inline bool conv_balance_parse(const char* s, long total_col_tiles, int wm, int wn, ConvBalancePlan* out) {
    if (!s || !*s) return false;
    long bulk = 0;
    const char* c = s;
    if (*c < '0' || *c > '9') return false;
    for (; *c >= '0' && *c <= '9'; ++c) bulk = bulk < (1L << 40) ? bulk * 10 + (*c - '0') : bulk;
    if (*c++ != ':') return false;
    int fwn = 0;
    if (c[0] == '3' && c[1] == '2' && c[2] == 'x' && c[3] == '6' && c[4] == '4' && !c[5]) fwn = 2;
    else if (c[0] == '3' && c[1] == '2' && c[2] == 'x' && c[3] == '3' && c[4] == '2' && !c[5]) fwn = 1;
    else return false;
    if (fwn > wn || 1 * fwn >= wm * wn) return false;
    if (bulk > total_col_tiles) bulk = total_col_tiles;
    bulk = bulk / 8 * 8;
    if (bulk >= total_col_tiles) *out = ConvBalancePlan{total_col_tiles, 0, 0, 0, 0};   // no remainder: the single-shape grid
    else *out = ConvBalancePlan{bulk, 1, fwn, 0, 0};
    return true;
}
