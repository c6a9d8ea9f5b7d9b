"""The geometries of the tile-run tests (tests/test_band_tile_run_cpu.py walks the runs of every one on the host,
tests/test_gpu_band_tile_run.py runs the kernels on them): name -> (S, mask parameters, vid0, F, P, ctx, text_first).  Every case has a
video, so that heads of both kinds run on it: text behind the video (S = F * P + ctx, vid0 = 0) or in front of it (S = ctx + F * P,
vid0 = ctx) — the two placements of the oracle."""
from oracle import svg_oracle as O

F5, P600, CTX, L = 5, 600, 256, 64


def _band(S, band):
    return dict(real_len=S, band=band, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)


def geometry(name):
    V = F5 * P600
    model, _, arg = name.partition("_")
    if model == "hy":             # hy_128 / hy_640 / hy_1536: text behind the video, padding behind the prompt
        S = V + CTX
        return S, dict(O.hy_band_params(S, CTX, L, F5, P600, 1.0), band=int(arg)), 0, F5, P600, CTX, False
    if model == "wan":            # no text; the first frame's columns are full
        return V, dict(O.wan_band_params(V, F5, P600, 1.0), band=int(arg)), 0, F5, P600, 0, False
    if model == "cog":            # text first: full rows and columns in front of the band
        S = V + CTX
        return S, dict(O.cog_band_params(S, CTX, F5, P600, 1.0), band=int(arg)), CTX, F5, P600, CTX, True
    if model == "cogsink":        # ... and the first frame's columns too: a column range that merges into the band's segment
        S = V + CTX
        return S, dict(O.cog_band_params(S, CTX, F5, P600, 1.0, attn_sink=True), band=int(arg)), CTX, F5, P600, CTX, True
    if model == "coglike":        # vid0 = 226, F = 3, P = 272: S = 1042 is no multiple of 64, the last q-tile has 18 rows
        F_, P_, c = 3, 272, 226
        S = c + F_ * P_
        return S, dict(O.cog_band_params(S, c, F_, P_, 1.0), band=int(arg)), c, F_, P_, c, True
    if model == "dense":          # band = S + 1: the run covers a segment; dense_valid: two segments, rows and keys behind real_len
        S = V + CTX
        return S, O.dense_band_params(S, V + L if arg == "valid" else None), 0, F5, P600, CTX, False
    if model == "last16":         # S = 1040 = 4 * 256 + 16: a last q-tile of 16 rows (waves 1 .. 7 idle), no multiple of 64; text first
        return 1040, _band(1040, 300), 100, 4, 235, 100, True
    if model == "ragged":         # S = 1001, text behind the video: the last key tile straddles S and the end of the video lies inside a tile
        return 1001, _band(1001, 330), 0, 4, 200, 201, False
    if model == "short":          # short_97 / short_161 / short_225: runs of no tile or one; text first, S = 1100
        return 1100, _band(1100, int(arg)), 100, 4, 250, 100, True
    if model == "few":            # few_3 / few_4 / few_5: that many key tiles, around dist + 2 of both wave halves; the video is the sequence
        n = int(arg)
        return 64 * n, O.dense_band_params(64 * n), 0, n, 64, 0, False
    raise ValueError(name)


MODEL_CASES = [f"{m}_{b}" for m in ("hy", "wan", "cog", "cogsink") for b in (128, 640, 1536)]
EDGE_CASES = ["coglike_128", "coglike_384", "dense_all", "dense_valid", "last16", "ragged", "short_97", "short_161", "short_225",
              "few_3", "few_4", "few_5"]
ALL_CASES = MODEL_CASES + EDGE_CASES
# a long run, a run of at most one tile, a ragged sequence with a 16-row last q-tile: for the entries beside the plain one
ENTRY_CASES = ["hy_640", "cogsink_640", "short_161", "last16"]
