"""Model check of which wave takes which look-back voice in the single-pass launches: a restatement, in Python, of the index
arithmetic of

- the host's waves per voice and grid (saugns_amd/csrc/hip_backend.hip:713-727, look_wpv_ and look_inside_; 1028-1029, grid2);
- fast_kernel<T, 2>'s mapping of waves to the voices of vlists[1] (k_fast_voice.h:556-584);
- duo_kernel's split of a workgroup's waves and its mapping (k_fast_voice.h:640-672: lw, wpv, j0, cs; SAU_AMD_DUO_LW forces lw);
- fast_voice's place of a voice's waves and rings in LDS (k_fast_voice.h:152-156: w0, look_lds, lk_base), with the rings as
  lookback32 / lookback64 address them (k_fast_group.h:247, 529: lk_base + scan slot x 2 x 64, a second half 64 words on).

Enumerated over grids of 1 to 256 workgroups, 2 to 14 and 16 look-back waves of a workgroup, 1 to 5000 look-back voices (sampled),
1 to 64 row groups and beyond, with the HBM words of the spread look-back there or not. Checked for every wave: every look-back voice
is rendered by exactly wpv waves, group phases cs = 0 .. wpv - 1 once each; a voice that looks back through rings in LDS has all its
waves in one workgroup, at local indices [w0, w0 + wpv); the rings of the voices of one workgroup do not overlap and lie inside
LOOK_LDS_BYTES; a voice of several waves that has no ring in LDS exists only where the words in HBM do; and a voice of several waves
is a wave's only one (j == j0: a second round would find the ring of the voice before it, and a w0 computed from j, not from the
wave's own slot). The last test feeds the model a second round by force and shows that it notices. CPU only."""
import numpy as np
import pytest

W = 16                 # waves of a 1024-thread workgroup
FAST_MAX_SCAN = 8      # k_fast_types.h: running-sum oscillators of a voice, each with a ring in LDS
LOOK_LDS_WORDS = FAST_MAX_SCAN * 2 * 64  # LOOK_LDS_BYTES / 8: one word per thread


def _round_pow2_16(w):
    return 16 if w >= 16 else 8 if w >= 8 else 4 if w >= 4 else 2 if w >= 2 else 1


def host_look(fk_grid, n_voices, groups, words_real, no_lds=False):
    """hip_backend.hip:713-727 and 1028-1029: (look_wpv_, look_inside_, grid2) of the look-back launch apart"""
    wpv = (fk_grid * 16) // n_voices
    wpv = min(wpv, 64, groups)
    wpv = max(wpv, 1)
    is_inside = lambda w: w <= 16 and 16 % w == 0 and not no_lds
    if not words_real and not is_inside(wpv) and not no_lds:
        wpv = 16 if wpv > 16 else 8 if wpv > 8 else 4 if wpv > 4 else 2
    inside = not words_real and is_inside(wpv)
    waves = n_voices * (min(groups, 64) if words_real else wpv)
    grid2 = fk_grid if waves > fk_grid * 16 else (waves + 15) // 16
    return wpv, inside, max(grid2, 1)


def fast_kernel_look(grid, n_look, look_wpv, look_groups, words_real, spread=False):
    """k_fast_voice.h:556-584 (SCAN == 2): per wave g, (j0, cs, wpv, slots_v) -- or None for a wave that returns"""
    total_waves = grid * W
    wpv = look_wpv
    if words_real:
        wpv = min(total_waves // n_look, look_groups)
        wpv = 64 if wpv >= 64 else 32 if wpv >= 32 else _round_pow2_16(wpv)
    slots_v = total_waves // wpv
    sp = wpv >= 32 and spread
    g = np.arange(total_waves)
    j0 = g % slots_v if sp else g // wpv
    cs = g // slots_v if sp else g % wpv
    return g, j0, cs, wpv, slots_v, W


def duo_look(grid, lw, n_look, look_groups):
    """k_fast_voice.h:640-672: the look-back waves 0 .. lw - 1 of every workgroup; g numbers them across the launch"""
    total_waves = grid * lw
    wpv = min(total_waves // n_look, look_groups)
    wpv = 64 if wpv >= 64 else wpv if wpv > 16 else _round_pow2_16(wpv)
    slots_v = total_waves // wpv
    g = np.arange(total_waves)
    return g, g // wpv, g % wpv, wpv, slots_v, lw


def duo_lw(n_look, n_cf, forced=0):
    """k_fast_voice.h:644-649: look-back waves of a workgroup's 16"""
    lw = W if n_cf == 0 else 0
    if n_look and n_cf:
        lw = (16 * n_look + (n_look + n_cf) // 2) // (n_look + n_cf)
        lw = min(max(lw, 2), 14)
        if forced & 15:
            lw = forced & 15
    return lw


def assign(g, j0, cs, wpv, slots_v, wg_waves, n_look, no_lds=False):
    """Every (wave, voice) pair the launch renders -- voices j0, j0 + slots_v, ... -- with what fast_voice derives for it
    (k_fast_voice.h:152-156)"""
    step = slots_v
    keep = (j0 < step) & (cs < wpv)
    g, j0, cs = g[keep], j0[keep], cs[keep]
    rows = []
    r = 0
    while True:
        j = j0 + r * step
        on = j < n_look
        if not on.any():
            break
        rows.append((g[on], j0[on], j[on], cs[on]))
        r += 1
    if not rows:
        return None
    g, j0, j, cs = (np.concatenate(c) for c in zip(*rows))
    w0 = (j * wpv) % wg_waves
    look_lds = (wpv >= 2) & (w0 + wpv <= wg_waves) & (not no_lds)
    return dict(g=g, j0=j0, j=j, cs=cs, w0=w0, look_lds=look_lds, block=g // wg_waves, local=g % wg_waves)


def problems(a, wpv, n_look, wg_waves, words_real):
    """what is wrong with an assignment, as a list of sentences (empty: nothing)"""
    out = []
    j, cs = a["j"], a["cs"]
    # every voice: exactly wpv waves, phases 0 .. wpv - 1 once each
    cnt = np.bincount(j * wpv + cs, minlength=n_look * wpv)
    if cnt.size != n_look * wpv or (cnt != 1).any():
        out.append(f"voices without exactly one wave per phase: {np.flatnonzero(cnt != 1)[:4] // wpv}")
    lds = a["look_lds"]
    if lds.any():
        jl, bl, ll, w0 = j[lds], a["block"][lds], a["local"][lds], a["w0"][lds]
        # one workgroup, local indices [w0, w0 + wpv)
        first = np.full(n_look, -1)
        first[jl] = bl
        if (first[jl] != bl).any():
            out.append(f"a voice with rings in LDS straddles workgroups: voices {np.unique(jl[first[jl] != bl])[:4]}")
        bad = (ll < w0) | (ll >= w0 + wpv)
        if bad.any():
            out.append(f"a voice's waves are not at [w0, w0 + wpv) in its workgroup: voices {np.unique(jl[bad])[:4]}")
        # rings: lk_base = lring + 4 w0, 4 wpv words, in every scan slot's two halves (k_fast_group.h: + slot * 128 (+ 64))
        end = (FAST_MAX_SCAN - 1) * 128 + 64 + (w0 + wpv) * 4
        if (end > LOOK_LDS_WORDS).any():
            out.append("a ring beyond LOOK_LDS_BYTES")
        # (voice by voice: its workgroup and w0 as its first wave has them)
        _, at = np.unique(jl, return_index=True)
        vb_, vw = bl[at], w0[at]
        o = np.lexsort((vw, vb_))
        vb_, vw = vb_[o], vw[o]
        if ((vb_[1:] == vb_[:-1]) & (vw[1:] - vw[:-1] < wpv)).any():
            out.append("the rings of two voices of one workgroup overlap")
    if wpv >= 2:
        if (a["j"] != a["j0"]).any():
            out.append("a wave takes a second voice while voices have several waves")
        if not words_real and (~lds).any():
            out.append("a voice of several waves without rings in LDS where no words in HBM exist")
    return out


def _voice_counts(rng, top):
    """look-back voice counts: the small ones all, edges of the waves' division, a sample of the rest"""
    n = set(range(1, 18)) | {31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 5000}
    n |= set(int(x) for x in rng.integers(1, top + 1, 12))
    return sorted(x for x in n if x <= top)


GROUPS = [1, 2, 3, 5, 7, 8, 15, 16, 17, 31, 33, 63, 64, 65, 200, 4000]


@pytest.mark.parametrize("lw", list(range(2, 15)) + [16])
def test_duo_kernel_waves_take_every_look_back_voice_once(lw):
    """duo_kernel at every grid 1 .. 256 and split lw: each voice's phases once, rings in LDS only within one workgroup"""
    rng = np.random.default_rng(4400 + lw)
    checked = 0
    for grid in range(1, 257):
        for n_look in _voice_counts(rng, 5000)[:: 3 if grid % 5 else 1]:
            for groups in GROUPS[grid % 3::3] if grid % 7 else GROUPS:
                g, j0, cs, wpv, slots_v, wg = duo_look(grid, lw, n_look, groups)
                a = assign(g, j0, cs, wpv, slots_v, wg, n_look)
                assert a is not None, (grid, lw, n_look, groups)
                p = problems(a, wpv, n_look, wg, True)
                assert not p, (grid, lw, n_look, groups, wpv, p)
                checked += 1
    assert checked > 3000


# (SAU_AMD_LOOK_SPREAD acts only on voices of 32 or 64 waves: where the words in HBM exist)
@pytest.mark.parametrize("words_real, spread", [(True, False), (True, True), (False, False)])
def test_fast_kernel_look_back_waves_take_every_voice_once(words_real, spread):
    """fast_kernel<T, 2> with the host's waves per voice and grid: the segment's voices of which analyze_kernel finds n_look to
    take the look-back, at every device size 1 .. 256 CUs, with and without the words in HBM"""
    rng = np.random.default_rng(4500 + 2 * words_real + spread)
    checked = 0
    for fk_grid in range(1, 257):
        for n_voices in _voice_counts(rng, 5000)[:: 3 if fk_grid % 4 else 1]:
            for groups in GROUPS[fk_grid % 2::2]:
                look_wpv, inside, grid2 = host_look(fk_grid, n_voices, groups, words_real)
                if not words_real:
                    assert inside, (fk_grid, n_voices, groups, look_wpv)  # (no words, so every voice keeps to its workgroup)
                for n_look in {1, n_voices, max(1, n_voices // 3), max(1, n_voices - 1)}:
                    g, j0, cs, wpv, slots_v, wg = fast_kernel_look(grid2, n_look, look_wpv, groups, words_real, spread)
                    a = assign(g, j0, cs, wpv, slots_v, wg, n_look)
                    assert a is not None
                    p = problems(a, wpv, n_look, wg, words_real)
                    assert not p, (fk_grid, n_voices, n_look, groups, grid2, wpv, p)
                    checked += 1
    assert checked > 3000


def test_duo_split_follows_the_lists_and_the_forced_value():
    """duo_lw: by the lists' lengths, 2 .. 14 with both kinds present, every wave to the one kind present, SAU_AMD_DUO_LW over all"""
    assert duo_lw(5, 0) == 16
    assert duo_lw(1, 1000) == 2 and duo_lw(1000, 1) == 14 and duo_lw(64, 64) == 8
    for forced in (3, 7, 15):
        assert duo_lw(64, 64, forced) == forced
    for nl in range(1, 300, 7):
        for nc in range(1, 300, 11):
            assert 2 <= duo_lw(nl, nc) <= 14


def test_second_rounds_only_with_one_wave_per_voice():
    """Where a wave does take several voices (more look-back voices than waves), each of them has one wave and no ring in LDS"""
    for grid, lw, n_look in ((1, 2, 5000), (37, 7, 4000), (255, 3, 1000), (16, 16, 257)):
        g, j0, cs, wpv, slots_v, wg = duo_look(grid, lw, n_look, 64)
        a = assign(g, j0, cs, wpv, slots_v, wg, n_look)
        assert wpv == 1 and (a["j"] != a["j0"]).any() and not a["look_lds"].any()
        assert not problems(a, wpv, n_look, wg, True)


def test_a_forced_second_round_is_caught():
    """Negative control: grid 255, lw 7, wpv 4 as ADVICE imagined it -- fewer voice slots than voices, so that waves take a second
    voice, whose w0 the kernel would derive from j. The model sees the voice whose waves straddle two workgroups (or sit elsewhere
    than at [w0, w0 + wpv)) -- it has teeth -- while the same launch in one round has nothing to report."""
    grid, lw, n_look = 255, 7, 500
    g = np.arange(grid * lw)
    wpv = 4
    slots_v = grid * lw // wpv  # 446 voice slots for 500 voices: waves 0 .. 215 take a second voice
    assert duo_look(grid, lw, n_look, 64)[3] == 2  # (what the kernel picks: 1785 // 500 = 3, rounded down)
    a = assign(g, g // wpv, g % wpv, wpv, slots_v, lw, slots_v)
    assert not problems(a, wpv, slots_v, lw, True)
    a = assign(g, g // wpv, g % wpv, wpv, slots_v, lw, n_look)
    p = problems(a, wpv, n_look, lw, True)
    assert any("straddles" in s or "[w0, w0 + wpv)" in s for s in p), p
    assert any("second voice" in s for s in p), p
