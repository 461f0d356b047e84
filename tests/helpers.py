"""Shared comparison helpers: the HIP engine vs the oracle (tests only)."""
from __future__ import annotations

import numpy as np

from oracle import cref


def assert_index_equal(eng, oix, ctx: str = "") -> None:
    st = eng.stats()
    assert st.n_total == oix.n_total, (ctx, "n_total", st.n_total, oix.n_total)
    assert st.n_dropped == oix.n_dropped, (ctx, "n_dropped")
    assert st.n_kept == oix.n_kept, (ctx, "n_kept")
    assert st.n_unique == oix.n_unique, (ctx, "n_unique", st.n_unique, oix.n_unique)
    assert st.n_keys == oix.n_keys, (ctx, "n_keys", st.n_keys, oix.n_keys)
    g = eng.export()
    o = oix.unique()
    # masses bit-exact (compare the float64 bit patterns)
    assert np.array_equal(g["mass"].view(np.uint64), o["mass"].view(np.uint64)), (ctx, "mass")
    for k in ("prot_id", "offset", "length", "occ_off", "occ_prot"):
        a, b = g[k], o[k]
        if not np.array_equal(a.astype(np.uint64), b.astype(np.uint64)):
            bad = np.nonzero(a.astype(np.uint64) != b.astype(np.uint64))[0][:5]
            raise AssertionError(f"{ctx}: {k} differs at {bad}: gpu={a[bad]} oracle={b[bad]}")
    assert np.array_equal(eng.entry_keys(), oix.entry_keys()), (ctx, "entry keys")


def query_masses(oix, n: int, seed: int = 7, ppm: float = 20.0):
    """SURVEY.md §8(d) query mix: 90 % indexed masses x (1 + N(0, 5 ppm)),
    10 % uniform on [500, 6000]; tolerance = getToleranceInDalton(m, ppm)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    u = oix.unique()["mass"] if hasattr(oix, "unique") else oix
    k = int(n * 0.9)
    m = np.empty(n, np.float64)
    if u.shape[0]:
        m[:k] = u[rng.integers(0, u.shape[0], k)] * (1 + rng.normal(0, 5e-6, k))
    else:
        m[:k] = rng.uniform(500, 6000, k)
    m[k:] = rng.uniform(500, 6000, n - k)
    tol = m * (1 - 1 / (ppm / 1000000 + 1))
    return m, tol


def assert_queries_equal(eng, oix, masses, tols, ctx: str = "") -> None:
    first, count = eng.query(masses, tols)
    of, oc = oix.query_batch(masses, tols)
    bad = np.nonzero((count != oc) | ((count > 0) & (first != of)))[0]
    assert bad.shape[0] == 0, (ctx, "query mismatch", bad[:5], masses[bad[:5]], first[bad[:5]], of[bad[:5]],
                               count[bad[:5]], oc[bad[:5]])


def tag_collision_proteins():
    """Proteins whose tryptic peptides include isobaric permutations with
    bit-identical fp64 MH+ AND equal 16-bit tag (pairs and a triple), repeated
    in mixed order, so the equal-(mass, tag) groups hold different strings and
    the pinned first-appearance order is exercised."""
    import collections
    import itertools

    from dbindex_amd.params import DBIndexSearchParams, calculate_mass
    from oracle.pyref import peptide_tag

    prm = DBIndexSearchParams.trypsin(0)
    groups = collections.defaultdict(list)
    for perm in itertools.permutations("ACDEFGHM"):
        s = "".join(perm) + "K"
        groups[(np.float64(calculate_mass(s, prm)).view(np.uint64).item(), peptide_tag(s))].append(s)
    pairs = [v for v in groups.values() if len(v) == 2][:40]
    triples = [v for v in groups.values() if len(v) >= 3][:10]
    prots = []
    for a, b in pairs:
        prots.append(b + a + "WWWWWWK" + b)
        prots.append(a + a + b + "GGGGGGGR" + a)
    for t in triples:
        prots.append(t[2] + t[0] + t[1] + t[0])
        prots.append(t[1] * 5 + t[2])
    return prots


# ---------------------------------------------------------------------------
# Seam constructions (tests/test_seams_gpu.py, and their CPU twins in
# tests/test_oracle.py).  The constants restate the engine's geometry
# (dbindex_amd/csrc): they are where the tests aim, not inputs of the engine.
# ---------------------------------------------------------------------------
TILE = 4096          # DIGEST_TILE: starts per digest block
HORIZON = 128        # LD_HORIZON: positions a lean walk reads from LDS
PST_CAP = 192        # protein starts of a tile window kept in LDS
HEAVY = 30000.0      # table mass of the filler letter: above every maxMH used here

# K/R sites, KP and RP (no cleavage under nocut="P"), adjacent KR and RR, a
# peptide shorter than MIN_PEP_LENGTH (AGK), and a C-terminal tail without K/R
SEAM_PROBE = "MAGDEFKPLSTVNRPWYHEQKRAGKCDEFGHILRRSSTTVVWYKLMNQAGDEFHIRGASPVTCLINDQEMHFYW"


def seam_shifts(probe: str = SEAM_PROBE):
    """Every s in [-len(probe)-2, +2] (each site, start and end of the probe on
    tile positions 4095 / 4096 / 4097 and inside the 16-residue pre-context),
    the 64-position bit-map word edge and the 128-position horizon edge."""
    s = set(range(-len(probe) - 2, 3)) | {-65, -64, -63} | set(range(-130, -125))
    return sorted(s)


def seam_params(prm):
    """prm with the filler letter X made heavier than maxMH: every peptide
    containing it is dropped by the walk."""
    prm.residue_mass["X"] = HEAVY
    return prm


def _ordinary(rng, n: int) -> str:
    return "".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), n))


def seam_proteome(shifts, probe: str = SEAM_PROBE, tail: int = 200, extra=()):
    """(seqs, probe_starts): the probe once per tile pair, at global residue
    4096*(2i+1) + shifts[i], each behind a filler protein of exactly the needed
    length (X's, then `tail` ordinary residues, so peptides of the filler's
    end and of the probe cross the tile edge from both sides); `extra`
    proteins follow the last probe."""
    rng = np.random.default_rng(41)
    seqs, starts, pos = [], [], 0
    for i, s in enumerate(shifts):
        at = TILE * (2 * i + 1) + s
        n = at - pos
        assert n > tail
        seqs.append("X" * (n - tail) + _ordinary(rng, tail))
        seqs.append(probe)
        starts.append(at)
        pos = at + len(probe)
    seqs += list(extra)
    return seqs, starts


def horizon_proteins():
    """[(d, kind, protein)]: glycine runs (57 Da: far below a 20000-Da maxMH)
    whose distance from start 0 to its next stop ("stop": G*d + K...) or to
    its last candidate end under two missed cleavages ("last": two early
    stops, then the third at d) is d = 126..130 positions -- either side of
    the 128-position walk horizon."""
    out = []
    for d in range(HORIZON - 2, HORIZON + 3):
        out.append((d, "stop", "G" * d + "K" + "AAAAAAR"))
        out.append((d, "last", "AAAAAAK" + "GGGGGGR" + "G" * (d - 14) + "K" + "GGGGGGGW"))
    return out


def horizon_proteome(extra=()):
    """(seqs, starts): every horizon protein as it is (wherever it falls) and
    again with its start on tile positions 3967, 3968 and 3969 (start + 128 =
    the tile's end), one tile each, behind an exact filler; `extra` proteins
    follow."""
    rng = np.random.default_rng(43)
    seqs, starts, pos = [], [], 0
    for d, kind, p in horizon_proteins():
        seqs.append(p)
        pos += len(p)
    for d, kind, p in horizon_proteins():
        for q in (TILE - HORIZON - 1, TILE - HORIZON, TILE - HORIZON + 1):
            t = (pos + TILE - 1) // TILE + 1  # a tile the filler can reach with room for its tail
            at = TILE * t + q
            n = at - pos
            seqs.append("X" * (n - 100) + _ordinary(rng, 100))
            seqs.append(p)
            starts.append(at)
            pos = at + len(p)
    seqs += list(extra)
    return seqs, starts


def pst_proteome(counts=tuple(range(170, 200)), empties: bool = False):
    """(seqs, tile0, counts): one tile per entry of `counts`, holding exactly
    that many protein starts (short proteins of one fixed length ending in K
    or R, the last taking the rest of the tile; with `empties`, an empty
    protein at the tile's first position as well -- two starts at one
    position).  The digest keeps a tile window's protein starts in LDS when
    they fit PST_CAP = 192; the window reaches past the tile on both sides, so
    the sweep crosses the capacity for any window, and the tiles of exactly
    191 / 192 / 193 starts are among them."""
    rng = np.random.default_rng(47)
    seqs = ["X" * (TILE - 300) + _ordinary(rng, 300)]  # tile 0; the sweep starts on a tile edge
    for n in counts:
        k = n - 1 if empties else n
        L = TILE // k
        if empties:
            seqs.append("")
        for j in range(k):
            ln = L if j < k - 1 else TILE - L * (k - 1)
            seqs.append(_ordinary(rng, ln - 1) + "KR"[j & 1])
    return seqs, 1, list(counts)


def perm_family():
    """The largest group of "ACDE" + perm("MNPQS") + "FGHK" with bit-identical
    MH+ and equal 16-bit tag under trypsin(0) (the tag hashes the length and
    the first and last four residues only): a whole family of different
    strings in one equal-(mass, tag) group."""
    import collections
    import itertools

    from dbindex_amd.params import DBIndexSearchParams, calculate_mass
    from oracle.pyref import peptide_tag

    prm = DBIndexSearchParams.trypsin(0)
    groups = collections.defaultdict(list)
    for perm in itertools.permutations("MNPQS"):
        s = "ACDE" + "".join(perm) + "FGHK"
        groups[(np.float64(calculate_mass(s, prm)).view(np.uint64).item(), peptide_tag(s))].append(s)
    return max(groups.values(), key=len)


def family_proteins(k: int, total: int, seed: int = 0):
    """~total one-peptide proteins: k strings of the family, total // k copies
    of each (at least one), in an order shuffled by a seeded generator."""
    fam = perm_family()[:k]
    assert len(fam) == k
    seqs = fam * max(total // k, 1)
    rng = np.random.default_rng(100 + seed)
    return [seqs[i] for i in rng.permutation(len(seqs))]


# a few dozen peptides several Da from one another and from the spikes below
UNRELATED = ["W" * k + "AAAAAK" for k in range(1, 25)]


def isobaric_pair():
    """Two permutations of ACDEFGHM + K with bit-identical MH+ and different
    16-bit tags (one mass, two tags)."""
    import collections
    import itertools

    from dbindex_amd.params import DBIndexSearchParams, calculate_mass
    from oracle.pyref import peptide_tag

    prm = DBIndexSearchParams.trypsin(0)
    first = {}
    for perm in itertools.permutations("ACDEFGHM"):
        s = "".join(perm) + "K"
        key = np.float64(calculate_mass(s, prm)).view(np.uint64).item()
        if key in first and peptide_tag(first[key]) != peptide_tag(s):
            return first[key], s
        first.setdefault(key, s)
    raise AssertionError("no isobaric pair with different tags")


def capacity_proteins(shape: str, size: int, prm):
    """One mass bin of exactly `size` records under trypsin(0) (one tryptic
    peptide of at least MIN_PEP_LENGTH per protein), beside UNRELATED:
    "one": one string; "two": two isobaric strings of different tags,
    interleaved; "many": the near-isobaric construction of
    test_multi_mass_wide_bins (a 3.7-uDa letter repeated 0..17 times: ~50
    masses within 0.07 mDa) with, from 200 records on, one (mass, tag) run of
    exactly 32 and one of exactly 33 records (18 and 19 repeats: masses of
    their own)."""
    if shape == "one":
        seqs = ["ACDEFGHMK"] * size
    elif shape == "two":
        a, b = isobaric_pair()
        seqs = [a if i % 2 == 0 else b for i in range(size)]
    else:
        prm.residue_mass.update({"U": 0.0000037})
        rng = np.random.default_rng(9)

        def one(k):
            core = list("GGAWDEFH") + ["U"] * k
            rng.shuffle(core)
            return "MR" + "".join(core) + "K"

        runs = [one(18)] * 32 + [one(19)] * 33 if size >= 200 else []
        seqs = [one(int(rng.integers(0, 18))) for _ in range(size - len(runs))]
        for r in runs:
            seqs.insert(int(rng.integers(0, len(seqs) + 1)), r)
    assert len(seqs) == size
    half = len(UNRELATED) // 2
    return UNRELATED[:half] + seqs + UNRELATED[half:]


def with_exact_duplicates(d, dup_idx):
    """(mass, pid, offset, length) of a digest with the occurrences `dup_idx`
    given a second time right after the first (exact duplicates: addSequence
    called again for the same protein and offset), in cref.Index's order."""
    idx = np.sort(np.concatenate([np.arange(d.mass.shape[0]), np.asarray(dup_idx, np.int64)]), kind="stable")
    return d.mass[idx], d.pid[idx], d.offset[idx], d.length[idx]
