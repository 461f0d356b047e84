"""GPU: the engine's seams.  Random proteomes and round sizes hit a given
alignment or capacity only by luck; here one known structure is put at every
alignment against the digest's geometry (tiles of 4096 starts, 16 residues of
N-terminal context, the 128-position walk horizon, 64-position bit-map words,
the 192-entry protein-start list), one mass bin is built at n-1 / n / n+1
records for every capacity that selects a sort kernel or sizes an LDS array,
and equal-(mass, tag) groups hold up to 70 different strings.  Everything is
compared bit-exactly with the oracle through the C-ABI, cold, warm and warm
again (reference: DBIndexer.java:237-405,
DBIndexStoreSQLiteByteIndexMerge.java:620-719).  The generators live in
tests/helpers.py; tests/test_oracle.py pins the oracle's two restatements on
the same constructions.

Run on an MI355X:  python -m pytest tests/test_seams_gpu.py -m gpu -q
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from dbindex_amd import fasta
from dbindex_amd.params import DBIndexSearchParams, calculate_mass
from oracle import cref
from tests import helpers as H
from tests.helpers import assert_index_equal, assert_queries_equal, query_masses

pytestmark = pytest.mark.gpu

CHUNK_CAP, WAVE_SORT_LIMIT = 1984, 512  # dbindex_amd/csrc/dbi_internal.h


@pytest.fixture(scope="module")
def Engine():
    from dbindex_amd import _native
    from dbindex_amd.engine import Engine
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")
    return Engine


def _pack(seqs):
    return fasta.PackedProteins.from_sequences(seqs, [fasta.uniprot_header(i) for i in range(len(seqs))])


def _stage_bytes(eng, name):
    return sum(b for n, _, b in eng.stage_times() if n == name)


def _check3(Engine, cp, pp, oix, ctx, options=None, nq=300, after=None):
    """Cold, warm and warm again on one engine, each equal to the oracle;
    after(eng, st, phase) sees every build.  Returns the last build's stage names."""
    m, t = query_masses(oix, nq)
    with Engine(cp, options=options) as eng:
        for phase in ("cold", "warm", "warm again"):
            st = eng.build(pp)
            assert_index_equal(eng, oix, f"{ctx} {options or {}} [{phase}]")
            assert_queries_equal(eng, oix, m, t, f"{ctx} {options or {}} [{phase}]")
            if after:
                after(eng, st, phase)
        return {n for n, _, _ in eng.stage_times()}


# --------------------------------------------------------------------------- A
@functools.lru_cache(maxsize=None)
def _human(n=1000):
    """Ordinary proteins beside the probes: enough records (DEPTH_MIN_RECS =
    2^14) that a warm lean build really takes depth bins."""
    return tuple(fasta.config("human").slice(0, n).sequences())


@functools.lru_cache(maxsize=None)
def _seam_pack(lean: bool):
    shifts = H.seam_shifts()
    seqs, starts = H.seam_proteome(shifts, extra=_human() if lean else ())
    pp = _pack(seqs)
    # the construction itself: probe i starts at 4096 (2i + 1) + s_i
    for i, s in enumerate(shifts):
        assert int(pp.offsets[2 * i + 1]) == H.TILE * (2 * i + 1) + s == starts[i]
        assert pp.sequence(2 * i + 1) == H.SEAM_PROBE
    return pp


X = H.seam_params
LEAN = [{}, {"depth_bins": 0}, {"part_stage": 0}]
DIGEST_SETS = [
    ("tryp0", X(DBIndexSearchParams.trypsin(0)), LEAN),
    ("tryp2", X(DBIndexSearchParams.trypsin(2)), LEAN),
    ("tryp2_nocutP", X(DBIndexSearchParams.trypsin(2, enzyme_nocut_residues="P")), LEAN),
    ("tryp3", X(DBIndexSearchParams.trypsin(3)), [{}]),  # not lean: max_missed + 2 > LD_ENDS
    ("semi1", X(DBIndexSearchParams.semi_tryptic(1)), [{}]),
    ("semi2", X(DBIndexSearchParams.semi_tryptic(2)), [{"semi_bounded": 1}, {"semi_bounded": 0}]),
    ("nonspec30", X(DBIndexSearchParams.non_specific(30)), [{}]),
    ("mand_K", X(DBIndexSearchParams.trypsin(2, mandatory_internal_aas="K")), [{}]),
]


@pytest.mark.parametrize("name,prm,optsets", DIGEST_SETS, ids=[d[0] for d in DIGEST_SETS])
def test_digest_seams(Engine, name, prm, optsets):
    """One probe protein (K/R sites, KP / RP, adjacent KR and RR, a peptide
    shorter than 6, a C-terminal tail without K/R) at every alignment
    s in [-len-2, +2], {-65..-63} and {-130..-126} against a tile edge: each of
    its cleavage sites, starts and ends on tile positions 4095 / 4096 / 4097,
    in the 16-residue pre-context, on a bit-map word edge and on the horizon
    edge.  The filler before each probe is a letter above maxMH (dropped by the
    walk) but for its last 200 residues.  The lean sets also run with depth
    bins off (the radix tail) and with the LDS record stage off; by default
    their warm builds take depth bins (ordinary proteins follow the probes)."""
    lean = optsets is LEAN
    pp = _seam_pack(lean)
    cp = prm.to_c()
    oix = cref.Index(cp, pp.residues, pp.offsets)
    assert oix.n_total > 2000
    for opts in optsets:
        names = _check3(Engine, cp, pp, oix, f"digest seams {name}", options=opts)
        if lean and not opts:
            assert oix.n_kept > 1 << 14
            assert "bin_scatter" in names, names
        if opts.get("depth_bins") == 0:
            assert "bin_scatter" not in names, names


@functools.lru_cache(maxsize=None)
def _horizon_pack(lean: bool):
    seqs, starts = H.horizon_proteome(extra=_human() if lean else ())
    pp = _pack(seqs)
    prots = H.horizon_proteins()
    k = len(prots)
    for j, at in enumerate(starts):  # 3 placements per protein: start + 128 = the tile's end, -1, +1
        i = k + 2 * j + 1
        assert int(pp.offsets[i]) == at and at % H.TILE == H.TILE - H.HORIZON - 1 + j % 3
        assert pp.sequence(i) == prots[j // 3][2]
    return pp


HORIZON_SETS = [
    ("tryp2", X(DBIndexSearchParams.trypsin(2, max_precursor_mass=20000.0)), LEAN),
    ("tryp0", X(DBIndexSearchParams.trypsin(0, max_precursor_mass=20000.0)), LEAN),
    ("semi2", X(DBIndexSearchParams.semi_tryptic(2, max_precursor_mass=20000.0)),
     [{"semi_bounded": 1}, {"semi_bounded": 0}]),
]


@pytest.mark.parametrize("name,prm,optsets", HORIZON_SETS, ids=[d[0] for d in HORIZON_SETS])
def test_horizon_probes(Engine, name, prm, optsets):
    """The 128-position horizon from inside: glycine runs under a 20000-Da
    maxMH whose distance from a start to its next stop, and to its last
    candidate end, is exactly 126, 127, 128, 129 and 130 positions
    (kth_bit_128 / first_bit_128 over two 64-bit words; 128 = horizon + 1 is
    not "closed"), each also with its start on tile positions 3967 / 3968 /
    3969, so the horizon's end is the tile's end."""
    # the probes are what they claim: start 0's first stop / last candidate end at d
    for d, kind, p in H.horizon_proteins():
        stops = [i for i, c in enumerate(p) if c in "KR"]
        assert (stops[0] if kind == "stop" else stops[2]) == d
    lean = optsets is LEAN
    pp = _horizon_pack(lean)
    cp = prm.to_c()
    oix = cref.Index(cp, pp.residues, pp.offsets)
    # every probe's long peptide is indexed (below maxMH, past the horizon for d >= 128)
    u = oix.unique()
    assert int(u["length"].max()) >= H.HORIZON + 3
    for opts in optsets:
        names = _check3(Engine, cp, pp, oix, f"horizon {name}", options=opts)
        if lean and not opts:
            assert "bin_scatter" in names, names


COUNT_SETS = [
    ("tryp2", DBIndexSearchParams.trypsin(2)),
    ("nonspec", DBIndexSearchParams.non_specific(30)),
    ("semi2", DBIndexSearchParams.semi_tryptic(2)),
    ("mandK", DBIndexSearchParams.trypsin(2, mandatory_internal_aas="K")),
    ("drop", DBIndexSearchParams.trypsin(4, index_factor=7, max_precursor_mass=7999.0)),
    ("drop13", DBIndexSearchParams.trypsin(4, index_factor=13, max_precursor_mass=7999.0)),
    ("fine", DBIndexSearchParams.trypsin(2, index_factor=64)),
    ("nonspec9", DBIndexSearchParams.non_specific(50, index_factor=9)),
    ("fine_nonspec", DBIndexSearchParams.non_specific(40, index_factor=64)),
]


@pytest.mark.parametrize("name,prm", COUNT_SETS, ids=[c[0] for c in COUNT_SETS])
def test_count_kernels_on_seams(Engine, name, prm):
    """dbi_count and dbi_count_buckets (the sets of test_count_buckets) over
    the seam proteome: the count kernels stage the same tiles, context and
    halo as the digests."""
    from dbindex_amd._native import DeviceBuffer
    pp = _seam_pack(False)
    cp = X(prm).to_c()
    want = cref.count_buckets(cp, pp.residues, pp.offsets)
    total = cref.count(cp, pp.residues, pp.offsets)
    assert total[0] > 2000
    d_res = DeviceBuffer.from_numpy(np.concatenate([pp.residues, np.zeros(16, np.uint8)]))
    d_off = DeviceBuffer.from_numpy(pp.offsets.astype(np.uint64))
    d_hist = DeviceBuffer.from_numpy(np.zeros(cp.index_factor + 1, np.uint64))
    with Engine(cp) as eng:
        assert eng.count_device(d_res.ptr, pp.n_residues, d_off.ptr, pp.n_proteins) == total, name
        assert eng.count_buckets_device(d_res.ptr, pp.n_residues, d_off.ptr, pp.n_proteins, d_hist.ptr) == total
    assert np.array_equal(d_hist.download(np.uint64, cp.index_factor + 1), want), name


@pytest.mark.parametrize("empties", [False, True], ids=["plain", "empty_first"])
@pytest.mark.parametrize("name,prm", [("tryp2", DBIndexSearchParams.trypsin(2)),
                                      ("semi1", DBIndexSearchParams.semi_tryptic(1))])
def test_protein_start_list_edge(Engine, name, prm, empties):
    """Tiles holding exactly 170 .. 199 protein starts, 191 / 192 / 193
    (PST_CAP = 192) among them: the digest keeps the offsets of the proteins
    its window touches in LDS when they fit (the window reaches past the tile
    on both sides, so which tile crosses the capacity depends on the kernel's
    window: the sweep covers either), else searches them in HBM.  With
    empty_first an empty protein sits at each tile's first position: two
    starts at one position, the map of starts cannot name the protein."""
    seqs, tile0, counts = H.pst_proteome(empties=empties)
    pp = _pack(seqs)
    per_tile = np.bincount((pp.offsets[:-1] // H.TILE).astype(np.int64))
    assert list(per_tile[tile0:tile0 + len(counts)]) == counts and {191, 192, 193} <= set(counts)
    if empties:
        for t in range(tile0, tile0 + len(counts)):
            i = int(np.searchsorted(pp.offsets, t * H.TILE))
            assert pp.offsets[i] == pp.offsets[i + 1] == t * H.TILE  # the empty protein opens the tile
    cp = X(prm).to_c()
    oix = cref.Index(cp, pp.residues, pp.offsets)
    names = _check3(Engine, cp, pp, oix, f"pst edge {name} empties={empties}")
    if name == "tryp2":
        assert "bin_scatter" in names, names


# --------------------------------------------------------------------------- B
CAPACITIES = [64, 512, 1024, 1984, 3968, 7936, 16384]


def _tier_asserts(size, ctx):
    def after(eng, st, phase):
        # BuildStats.n_big_bins: chunks above CHUNK_CAP
        assert (st.n_big_bins >= 1) == (size > CHUNK_CAP), (ctx, phase, size, st.n_big_bins)
        mid = _stage_bytes(eng, "chunk_sort_mid")
        print(f"{ctx} [{phase}]: n_big_bins={st.n_big_bins} chunk_sort_mid bytes={mid}")
        if size <= WAVE_SORT_LIMIT:
            assert mid == 0, (ctx, phase, mid)
        elif size == WAVE_SORT_LIMIT + 1:  # chunk_sort_mid's bytes: 32 x the records it sorted
            assert mid == 32 * size, (ctx, phase, mid)
    return after


@pytest.mark.parametrize("shape", ["one", "two", "many"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("n", CAPACITIES)
def test_capacity_seams(Engine, n, delta, shape):
    """One mass bin of exactly n-1, n and n+1 records beside two dozen
    unrelated peptides, for every capacity that selects a sort kernel or sizes
    an LDS array.  Which path the constants select (bin of `size` records):
      size <= 64 (RANK_MAX_RUN): equal-mass runs ranked inside the chunk sort;
        65 and up: the run goes to the wave's sort.  Not reported by the engine.
      size <= 512 (WAVE_SORT_LIMIT): one wave of k_chunk_sort; 513 and up:
        left out for chunk_sort_mid (its byte count: 0 at 512, 32 x 513 at 513).
      size <= 1024: chunk_sort_mid's small-block class; above: its large one.
      size <= 1984 (CHUNK_CAP): n_big_bins = 0; 1985: the big tier (n_big_bins >= 1).
      size <= 3968: the big tier's 512-thread class; above: the 1024-thread one.
      size <= 7936 (BIG_CAP, the 13-bit arrival index): LDS; above: the giant path.
      size <= 16384 (FB_LDS): the giant fallback sorts a segment in LDS; 16385:
        in global memory.  Not reported by the engine.
    Shapes: "one" string (the single-mass tag sort); "two" isobaric strings of
    different tags, interleaved; "many" masses within 0.07 mDa (the compact-key
    sorts) with one (mass, tag) run of exactly 32 and one of 33 (CK_RUN_MAX).
    The 3968 / 7936 rows also run with big_split 0 and 1; the 1984 / 7936 rows
    with big_side 0 and 1, there with ordinary proteins added so that the warm
    builds are depth-bin builds (the side stream is theirs)."""
    size = n + delta
    prm = DBIndexSearchParams.trypsin(0)
    seqs = H.capacity_proteins(shape, size, prm)
    pp = _pack(seqs)
    cp = prm.to_c()
    oix = cref.Index(cp, pp.residues, pp.offsets)
    assert oix.n_kept == size + len(H.UNRELATED)
    if shape == "many" and size >= 200:  # the two runs, each a peptide with a mass of its own
        per_unique = np.diff(oix.unique()["occ_off"]).tolist()
        assert per_unique.count(32) == 1 and per_unique.count(33) == 1 and max(per_unique) == 33
    optsets = [{}]
    if n in (3968, 7936):
        optsets += [{"big_split": 0}, {"big_split": 1}]
    ctx = f"capacity {shape} {size}"
    for opts in optsets:
        _check3(Engine, cp, pp, oix, ctx, options=opts, nq=100, after=_tier_asserts(size, ctx))
    if n in (1984, 7936):
        pp2 = _pack(seqs + list(_human()))
        oix2 = cref.Index(cp, pp2.residues, pp2.offsets)
        for opts in ({"big_side": 0}, {"big_side": 1}):
            names = _check3(Engine, cp, pp2, oix2, ctx + " + proteins", options=opts, nq=100)
            assert "bin_scatter" in names, names


@pytest.mark.parametrize("total", [1983, 1984, 1985])
def test_chunk_of_small_bins(Engine, total):
    """A chunk that is not one bin: four bins of at most 512 records (the
    lightest peptides of the index, 14 Da apart) whose total is exactly 1983,
    1984 and 1985 = CHUNK_CAP + 1.  With chunk_target 1536 chunk 0 ends with
    the bin that holds record 1535 -- the fourth -- so it is exactly these four
    bins (a chunk of small bins may reach T + 511): n_big_bins is 0 up to 1984
    and at least 1 at 1985, where the chunk no longer fits the LDS sort."""
    sizes = [500, 500, 500, total - 1500]
    assert max(sizes) <= WAVE_SORT_LIMIT
    peps = ["GGGGGGGK", "GGGGGGAK", "GGGGGAAK", "GGGGAAAK"]
    rng = np.random.default_rng(total)
    seqs = [p for p, k in zip(peps, sizes) for _ in range(k)]
    seqs = [seqs[i] for i in rng.permutation(len(seqs))] + H.UNRELATED
    pp = _pack(seqs)
    prm = DBIndexSearchParams.trypsin(0)
    cp = prm.to_c()
    oix = cref.Index(cp, pp.residues, pp.offsets)
    u = oix.unique()
    assert [int(x) for x in np.diff(u["occ_off"])[:4]] == sizes  # the four lightest uniques

    def after(eng, st, phase):
        assert (st.n_big_bins >= 1) == (total > CHUNK_CAP), (phase, total, st.n_big_bins)

    _check3(Engine, cp, pp, oix, f"small bins {total}", options={"chunk_target": 1536}, nq=100, after=after)


@pytest.mark.parametrize("size", [64, 65, 512, 513])
def test_capacity_seams_exact_duplicates(Engine, size):
    """The one-string rows at 64 / 65 and 512 / 513 through
    dbi_build_occurrences (the addSequence flow) with exact duplicate
    occurrences present -- the same protein, offset and length added twice:
    the ranks of equal records are broken by arrival (exact_dups), and no
    record may be lost.  A quarter of the bin's records are duplicates."""
    prm = DBIndexSearchParams.trypsin(0)
    ndup = size // 4
    seqs = H.capacity_proteins("one", size - ndup, prm)
    pp = _pack(seqs)
    cp = prm.to_c()
    d = cref.digest(cp, pp.residues, pp.offsets)
    spike_mass = calculate_mass("ACDEFGHMK", prm)
    spike = np.nonzero(d.mass == spike_mass)[0]
    assert spike.shape[0] == size - ndup
    occ = H.with_exact_duplicates(d, np.concatenate([spike[1:2 * ndup:2], np.arange(0, 6)]))
    assert int((occ[0] == spike_mass).sum()) == size
    oix = cref.Index(cp, pp.residues, pp.offsets, occurrences=occ)
    assert oix.n_kept == occ[0].shape[0]
    m, t = query_masses(oix, 100)
    with Engine(cp) as eng:
        for phase in ("cold", "warm", "warm again"):
            eng.build_occurrences(pp, *occ)
            assert_index_equal(eng, oix, f"occurrences {size} [{phase}]")
            assert_queries_equal(eng, oix, m, t, f"occurrences {size} [{phase}]")
            mid = _stage_bytes(eng, "chunk_sort_mid")
            assert (mid == 0) if size <= WAVE_SORT_LIMIT else (mid == 32 * size), (size, phase, mid)


# --------------------------------------------------------------------------- C
@pytest.mark.parametrize("total", [64, 300, 800, 3000, 6000, 10000, 17000])
@pytest.mark.parametrize("k", [2, 31, 32, 33, 70])
def test_many_string_groups(Engine, k, total):
    """One equal-(mass, tag) group of k different strings ("ACDE" + a
    permutation of MNPQS + "FGHK": the tag hashes the length and the first
    and last four residues only), total // k copies of each in a shuffled
    order, sized for every tier: <= 64 records (ranked bins; 70 strings need
    70 records: the wave sort), ~300 (wave sort), ~800 (mid), ~3 000 and ~6 000
    (big, both classes), ~10 000 (giant: fb_regroup keeps up to 32 strings in
    its 64-slot LDS table, 33 and 70 take the global path) and ~17 000 (beyond
    FB_LDS).  The unique order (first appearance within the group), the
    representative and the occurrence lists come through assert_index_equal."""
    fam = H.perm_family()
    assert len(fam) >= 70
    seqs = H.family_proteins(k, total, seed=k)
    pp = _pack(H.UNRELATED[:12] + seqs + H.UNRELATED[12:])
    for mc in (0, 2):
        cp = DBIndexSearchParams.trypsin(mc).to_c()
        oix = cref.Index(cp, pp.residues, pp.offsets)
        assert oix.n_unique == k + len(H.UNRELATED) and oix.n_kept == len(seqs) + len(H.UNRELATED)
        u = oix.unique()
        grp = np.nonzero(u["mass"] == calculate_mass(fam[0], DBIndexSearchParams.trypsin(mc)))[0]
        assert grp.shape[0] == k and np.array_equal(grp, np.arange(grp[0], grp[0] + k))
        _check3(Engine, cp, pp, oix, f"family k={k} total={total} mc={mc}", nq=100)


# --------------------------------------------------------------------------- D
STATE = "not built|no resident inputs"


def test_failed_build_leaves_no_stale_index(Engine):
    """dbi_build of text with '[' and no ']' fails after the upload has
    overwritten the resident residues: the handle must not keep answering from
    the previous index (its peptides would resolve against the wrong residues),
    and dbi_rebuild must not digest the '['-bearing text.  Every query-side
    call and rebuild raise the state error until the next good build."""
    from dbindex_amd._native import DBIndexStoreException
    base = fasta.config("1k")
    a, b = base.slice(0, 100), base.slice(0, 300)
    # other residues than A's, a little longer, ending in an unclosed formula
    bad = _pack(a.sequences()[::-1] + ["PEPTIDEK[C2H3NOAAAAAAK"])
    cp = DBIndexSearchParams.trypsin(2).to_c()
    oa, ob = cref.Index(cp, a.residues, a.offsets), cref.Index(cp, b.residues, b.offsets)
    m, t = query_masses(oa, 200)
    with Engine(cp) as eng:
        for first in (a, b):  # the failed build's text smaller, then larger than the resident buffer
            eng.build(first)
            assert_index_equal(eng, oa if first is a else ob, "before the failure")
            with pytest.raises(DBIndexStoreException, match="without"):
                eng.build(bad)
            for call in (lambda: eng.query(m, t), eng.export, lambda: eng.peptides([0, 1, 2]), eng.rebuild,
                         lambda: eng.query_csr(m, t)):
                with pytest.raises(DBIndexStoreException, match=STATE):
                    call()
            eng.build(a)
            assert_index_equal(eng, oa, "A after the failure")
            assert_queries_equal(eng, oa, m, t, "A after the failure")
            eng.build(b)
            assert_index_equal(eng, ob, "B after the failure")
            mb, tb = query_masses(ob, 200)
            assert_queries_equal(eng, ob, mb, tb, "B after the failure")
            eng.rebuild()
            assert_index_equal(eng, ob, "B rebuilt")


def test_failed_build_through_the_store():
    """The same through DBIndexStoreHip with device digestion (stopAddSeq
    hands the proteins' text to dbi_build): a second transaction that adds a
    protein with an unclosed '[' fails, and the store no longer answers from
    the first transaction's index."""
    from dbindex_amd import _native
    from dbindex_amd.store import DBIndexStoreHip
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")
    prm = DBIndexSearchParams.trypsin(2)
    pp = fasta.config("1k").slice(0, 100)
    oix = cref.Index(prm.to_c(), pp.residues, pp.offsets)
    u = oix.unique()
    mass = float(u["mass"][len(u["mass"]) // 2])
    st = DBIndexStoreHip(prm, device_digest=True)
    try:
        st.init("seams.fasta_dbindex")
        st.startAddSeq()
        for i, s in enumerate(pp.sequences()):
            st.addProteinDef(i, pp.defs[i], s)
        st.stopAddSeq()
        assert st.getTotalSeqCount() == oix.n_total
        assert len(st.getSequences(mass, 0.5)) == len(oix.query(mass, 0.5)) > 0
        st.startAddSeq()
        st.addProteinDef(pp.n_proteins, fasta.uniprot_header(pp.n_proteins), "PEPTIDEK[C2H3NOAAAAAAK")
        with pytest.raises(_native.DBIndexStoreException, match="without"):
            st.stopAddSeq()
        # the store's own contract for an engine that is not built: no index, no sequences
        # (a reference store without an index answers nothing) -- never the first index's
        assert st.getSequences(mass, 0.5) == [] and not st.indexExists()
        assert st.getNumberSequences() == 0 and st.getTotalSeqCount() == 0
    finally:
        st.close()
