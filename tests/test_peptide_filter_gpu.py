"""GPU: peptide filters in the device digest (dbi_set_peptide_filter;
DBIndexer.java:309-313).  Every expected index is the unfiltered oracle
digest without the occurrences whose peptide string isValid (restated in
tests/test_peptide_filter.py with ``str.count`` / ``re.search``) rejects --
the consequence that file pins against the literal loop -- built with
``cref.Index(occurrences=...)`` and compared bit-exactly.  Bucket drops of an
occurrences-built oracle index do not exist, so they are compared apart.

Run on an MI355X:  python -m pytest tests/test_peptide_filter_gpu.py -m gpu -q
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from dbindex_amd import fasta
from dbindex_amd.params import DBIndexSearchParams
from oracle import cref
from tests import helpers as H
from tests.helpers import assert_index_equal, assert_queries_equal, query_masses
from tests.test_peptide_filter import (FILTER_IDS, FILTERS, filtered_oracle, is_valid, literal_filtered_index,
                                       make_filter, strip_formulas, with_formulas)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    from dbindex_amd import _native
    from dbindex_amd.engine import Engine
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")
    return Engine


def _pack(seqs):
    return fasta.PackedProteins.from_sequences(seqs, [fasta.uniprot_header(i) for i in range(len(seqs))])


def _assert_filtered(eng, oix, n_drop, ctx):
    """The engine's index against the occurrences-built oracle index; the valid
    bucket drops (none in the oracle index) apart."""
    st = eng.stats()
    assert st.n_dropped == n_drop, (ctx, "n_dropped", st.n_dropped, n_drop)
    if n_drop == 0:
        assert_index_equal(eng, oix, ctx)
        return
    assert st.n_total == oix.n_total + n_drop, (ctx, "n_total")
    assert (st.n_kept, st.n_unique, st.n_keys) == (oix.n_kept, oix.n_unique, oix.n_keys), ctx
    g, o = eng.export(), oix.unique()
    assert np.array_equal(g["mass"].view(np.uint64), o["mass"].view(np.uint64)), (ctx, "mass")
    for k in ("prot_id", "offset", "length", "occ_off", "occ_prot"):
        assert np.array_equal(g[k].astype(np.uint64), o[k].astype(np.uint64)), (ctx, k)
    assert np.array_equal(eng.entry_keys(), oix.entry_keys()), (ctx, "entry keys")


def _unfiltered_unique(cp, pp, d):
    keep = ~d.dropped.astype(bool)
    return cref.Index(cp, pp.residues, pp.offsets,
                      occurrences=(d.mass[keep], d.pid[keep], d.offset[keep], d.length[keep])).n_unique


def _expect(cp, pp, filt, seqs=None):
    oix, n_drop, n_valid, d, valid = filtered_oracle(cp, pp, filt, seqs)
    assert 0 < oix.n_unique < _unfiltered_unique(cp, pp, d), "vacuous case"
    return oix, n_drop, n_valid, d, valid


# ------------------------------------------------------------------ parity
PARITY = [
    ("tryp2", DBIndexSearchParams.trypsin(2)),
    ("semi2", DBIndexSearchParams.semi_tryptic(2)),
    ("mandK", DBIndexSearchParams.trypsin(2, mandatory_internal_aas="K")),
    ("nonspec12", DBIndexSearchParams.non_specific(12)),
    ("drop", DBIndexSearchParams.trypsin(4, index_factor=7, max_precursor_mass=7999.0)),
]


@pytest.mark.parametrize("filt", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("name,prm", PARITY, ids=[c[0] for c in PARITY])
def test_filtered_build_parity(Engine, name, prm, filt):
    """300 random proteins: the index (cold and warm), 2000 queries, and
    dbi_count / dbi_count_buckets against the valid occurrences' counts."""
    from dbindex_amd._native import DeviceBuffer
    pp = fasta.config("1k").slice(0, 300)
    cp = prm.to_c()
    oix, n_drop, n_valid, d, valid = _expect(cp, pp, filt)
    if name == "drop" and filt != FILTERS[0]:  # (every peptide of these proteins past the last bucket holds an M)
        assert n_drop > 0
    m, t = query_masses(oix, 2000)
    with Engine(cp, peptide_filter=make_filter(filt)) as eng:
        for phase in ("cold", "warm"):
            eng.build(pp)
            _assert_filtered(eng, oix, n_drop, f"{name} {filt} [{phase}]")
            assert_queries_equal(eng, oix, m, t, f"{name} {filt} [{phase}]")
        d_res = DeviceBuffer.from_numpy(np.concatenate([pp.residues, np.zeros(16, np.uint8)]))
        d_off = DeviceBuffer.from_numpy(pp.offsets.astype(np.uint64))
        d_hist = DeviceBuffer.from_numpy(np.zeros(cp.index_factor + 1, np.uint64))
        assert eng.count_device(d_res.ptr, pp.n_residues, d_off.ptr, pp.n_proteins) == (n_valid, n_drop)
        assert eng.count_buckets_device(d_res.ptr, pp.n_residues, d_off.ptr, pp.n_proteins,
                                        d_hist.ptr) == (n_valid, n_drop)
        br = 8000 // cp.index_factor
        want = np.bincount(np.minimum(d.mass[valid].astype(np.int64) // br, cp.index_factor),
                           minlength=cp.index_factor + 1).astype(np.uint64)
        assert np.array_equal(d_hist.download(np.uint64, cp.index_factor + 1), want)
        # device-resident inputs take the same digest
        eng.build_device(d_res.ptr, pp.n_residues, d_off.ptr, pp.n_proteins)
        _assert_filtered(eng, oix, n_drop, f"{name} {filt} [build_device]")


# -------------------------------------------------------------------- KATs
def _kat_prm():
    # every substring of 6..30 residues is a candidate (each residue a cleavage site)
    return DBIndexSearchParams.non_specific(30, min_precursor_mass=300.0)


KATS = [
    # a motif that ends exactly at the start's 6th residue: no peptide of start 0 at all
    ("ends_at_6th", "N[^P][ST]", ["AAANGSAAAAAAW"], ["GSAAAA", "SAAAAAAW"], ["AAANGS", "AAANGSA"]),
    # a motif starting at s breaks start s; one starting at s - 1 does not
    ("starts_at_s", "N[^P][ST]", ["WNGSAAAAAAAA"], ["GSAAAA", "GSAAAAAAAA"], ["NGSAAA", "WNGSAA"]),
    # two alternatives of different lengths ending on one position: the shorter decides
    ("two_lengths", "WAAC|AC", ["KKWAACKKKKKK"], ["CKKKKK", "CKKKKKK"], ["ACKKKK", "AACKKK", "WAACKK", "KWAACK"]),
    # a motif split across two adjacent proteins is no match; the third protein holds a real one
    ("split", "N[^P][ST]", ["AAAAAAN", "GSAAAAAA", "WWNGSWWWW"], ["AAAAAAN", "GSAAAAAA", "GSWWWW"],
     ["WNGSWW", "NGSWWW"]),
    # proteins shorter than the motif (and than any peptide) beside ordinary ones
    ("short", "N[^P][ST]", ["NG", "S", "", "GS", "NGSAAAAAA", "AAAAAAA"], ["GSAAAA", "AAAAAAA"], ["NGSAAA"]),
    # aa as the first residue with num_max = 0: start 0 ends at once, start 1 walks
    ("aa_first", ("M", 0), ["MAAAAAAAK"], ["AAAAAAAK", "AAAAAA"], ["MAAAAA", "MAAAAAAAK"]),
    # the count restarts for each start (num_max = 2)
    ("restart", ("C", 2), ["CACACACAAAAA"], ["ACACAAAAA", "CACAAAAA", "CAAAAA"], ["CACACA", "ACACAC", "CACACAAAAA"]),
]


@pytest.mark.parametrize("name,filt,seqs,present,absent", KATS, ids=[k[0] for k in KATS])
def test_boundary_kats(Engine, name, filt, seqs, present, absent):
    prm = _kat_prm()
    cp = prm.to_c()
    pp = _pack(seqs)
    oix, n_drop, n_valid, d, valid = _expect(cp, pp, filt)
    plain = {seqs[p][o:o + n] for p, o, n in zip(d.pid.tolist(), d.offset.tolist(), d.length.tolist())}
    for s in present:
        assert s in plain and is_valid(filt, s), s
    for s in absent:
        assert s in plain and not is_valid(filt, s), s
    with Engine(cp, peptide_filter=make_filter(filt)) as eng:
        eng.build(pp)
        _assert_filtered(eng, oix, n_drop, name)
        g = eng.export()
        have = {seqs[p][o:o + n] for p, o, n in
                zip(g["prot_id"].tolist(), g["offset"].tolist(), g["length"].tolist())}
    assert have.issuperset(present), (name, set(present) - have)
    assert have.isdisjoint(absent), (name, have & set(absent))


# ------------------------------------------------------------------- seams
X = H.seam_params
SEAM_FILTERS = [("motif", "DEF|VN.P|TT"), ("count", ("E", 1))]
SEAM_SETS = [("tryp2", DBIndexSearchParams.trypsin(2)), ("semi1", DBIndexSearchParams.semi_tryptic(1)),
             ("nonspec30", DBIndexSearchParams.non_specific(30))]


@functools.lru_cache(maxsize=None)
def _seam_pack():
    seqs, _ = H.seam_proteome(H.seam_shifts())
    return _pack(seqs)


@pytest.mark.parametrize("fname,filt", SEAM_FILTERS, ids=[f[0] for f in SEAM_FILTERS])
@pytest.mark.parametrize("name,prm", SEAM_SETS, ids=[s[0] for s in SEAM_SETS])
def test_filter_on_tile_seams(Engine, name, prm, fname, filt):
    """The seam probe at every alignment against a tile edge, with motifs
    (three DEF, VNRP, TT) and counted residues inside it: matches straddle
    tile positions 4095 / 4096 / 4097 of the digest and of the motif
    pre-pass (tiles of 4096 ends behind a 15-residue halo)."""
    assert all(is_valid(filt, H.SEAM_PROBE[:k]) for k in range(4)) and not is_valid(filt, H.SEAM_PROBE)
    pp = _seam_pack()
    cp = X(prm).to_c()
    oix, n_drop, n_valid, d, valid = _expect(cp, pp, filt)
    assert n_valid > 1000
    m, t = query_masses(oix, 300)
    with Engine(cp, peptide_filter=make_filter(filt)) as eng:
        for phase in ("cold", "warm"):
            eng.build(pp)
            _assert_filtered(eng, oix, n_drop, f"seams {name} {fname} [{phase}]")
            assert_queries_equal(eng, oix, m, t, f"seams {name} {fname} [{phase}]")


def _overflow_proteome():
    """helpers.horizon_proteome, then glycine runs (57 Da a residue, far below
    the 20000-Da maxMH) that start 40 and 300 positions before a tile's end
    and hold a C after 320 and after 140 glycines: the walks from their first
    residues leave the staged window (the tile and 256 residues more) long
    before the filter ends them -- and would otherwise reach the K behind."""
    seqs, _ = H.horizon_proteome()
    pos = sum(len(s) for s in seqs)
    rng = np.random.default_rng(5)
    for back, run in ((40, 320), (300, 140), (1, 300)):
        t = (pos + H.TILE - 1) // H.TILE + 1
        at = H.TILE * t + H.TILE - back
        seqs.append("X" * (at - pos - 100) + H._ordinary(rng, 100))
        p = "G" * run + "CG" + "GGGK" + "AAAAAAR"
        seqs.append(p)
        pos = at + len(p)
    return seqs


@pytest.mark.parametrize("fname,filt", [("count", ("C", 0)), ("motif", "GCG|KAA")])
@pytest.mark.parametrize("name,prm", [("tryp2", DBIndexSearchParams.trypsin(2, max_precursor_mass=20000.0)),
                                      ("semi1", DBIndexSearchParams.semi_tryptic(1, max_precursor_mass=20000.0))])
def test_filter_breaks_past_the_staged_window(Engine, name, prm, fname, filt):
    """Glycine runs whose motif / counted residue lies past position 128 of
    the run and past the tile's staged window: the walk that meets it reads
    residues from HBM (walk_global_to), and breaks there."""
    seqs = _overflow_proteome()
    pp = _pack(seqs)
    cp = X(prm).to_c()
    oix, n_drop, n_valid, d, valid = _expect(cp, pp, filt)
    # the filter really removes peptides longer than the window's halo
    assert int(d.length[~valid].max()) > 300
    with Engine(cp, peptide_filter=make_filter(filt)) as eng:
        for phase in ("cold", "warm"):
            eng.build(pp)
            _assert_filtered(eng, oix, n_drop, f"overflow {name} {fname} [{phase}]")


# ------------------------------------------------------------ combinations
@pytest.mark.parametrize("filt", [FILTERS[1], FILTERS[3]], ids=[FILTER_IDS[1], FILTER_IDS[3]])
def test_filter_with_windows_rebuild(Engine, filt):
    """dbi_set_windows on a filtered, unbucketed engine: the window-filtered
    (re)build is the filtered oracle index restricted to the windows."""
    prm = DBIndexSearchParams.trypsin(2)
    pp = fasta.config("1k").slice(0, 300)
    cp = prm.to_c()
    oix, n_drop, _, _, _ = _expect(cp, pp, filt)
    assert n_drop == 0  # maxMH below the last bucket: the unbucketed index is the same
    o = oix.unique()
    um = o["mass"]
    rng = np.random.default_rng(5)
    with Engine(cp, peptide_filter=make_filter(filt)) as eng:
        eng.set_bucket_drop(False)
        for rep, k in enumerate((1, 7, 60)):
            m = um[rng.integers(0, um.shape[0], k)] + rng.normal(0, 0.01, k)
            t = rng.choice([0.0, 0.02, 0.5, 3.0], k)
            eng.set_windows(m, t)
            st = eng.build(pp) if rep == 0 else eng.rebuild()
            f = eng.export()
            sel = np.zeros(um.shape[0], bool)
            for a, b in zip(m - t, m + t):
                sel |= (um >= a) & (um <= b)
            ids = np.nonzero(sel)[0]
            assert st.n_unique == ids.shape[0] > 0, k
            assert np.array_equal(f["mass"].view(np.uint64), um[ids].view(np.uint64)), k
            for key in ("prot_id", "offset", "length"):
                assert np.array_equal(f[key], o[key][ids]), (k, key)
            occ = [o["occ_prot"][int(o["occ_off"][i]):int(o["occ_off"][i + 1])] for i in ids]
            assert np.array_equal(f["occ_prot"], np.concatenate(occ)), k
        eng.set_windows(on=False)  # windows off: the filter stays
        eng.rebuild()
        assert_index_equal(eng, oix, "windows off")


@pytest.mark.parametrize("filt", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("name,prm", [("tryp2", DBIndexSearchParams.trypsin(2)),
                                      ("semi1", DBIndexSearchParams.semi_tryptic(1))])
def test_filter_with_inline_ptms(Engine, name, prm, filt):
    """The PTM build: the filter sees the stripped residues (a formula step
    appends nothing to the peptide string).  Expected: the literal loop of
    tests/test_peptide_filter.py with the filter inside it (pinned there
    against the oracle without a filter) -- post-filtering the unfiltered
    digest is not the reference here: a walk the filter ends early leaves the
    formulas behind it to a later start, and may never reach an unknown
    element (first seen on the GPU: tryp2 ("M", 0), 90 proteins, 3335
    occurrences against the post-filter's 3320)."""
    seqs = with_formulas(fasta.config("1k").slice(0, 45).sequences())
    assert any("N[HPO3]GS" in s for s in seqs) and any("[Qx2]" in s for s in seqs)
    pp = _pack(seqs)
    cp = prm.to_c()
    oix, n_drop, n_occ = literal_filtered_index(prm, filt, pp, seqs)
    d = cref.digest(cp, pp.residues, pp.offsets)
    assert 0 < oix.n_unique < _unfiltered_unique(cp, pp, d), "vacuous case"
    if filt == "N[^P][ST]":  # the motif across the formula is seen: no peptide over N[HPO3]GS is left
        u = oix.unique()
        stripped = [strip_formulas(s) for s in seqs]
        assert not any("NGS" in stripped[p][o:o + n] for p, o, n in
                       zip(u["prot_id"].tolist(), u["offset"].tolist(), u["length"].tolist()))
    with Engine(cp, peptide_filter=make_filter(filt)) as eng:
        for phase in ("cold", "warm"):
            eng.build(pp)
            _assert_filtered(eng, oix, n_drop, f"ptm {name} {filt} [{phase}]")
            assert eng.stats().n_total == n_occ


@pytest.mark.parametrize("filt", [FILTERS[0], FILTERS[2]], ids=[FILTER_IDS[0], FILTER_IDS[2]])
def test_filter_with_local_shards(Engine, filt):
    """3 shards of one process over 500 proteins: every shard's digest
    (dbi_shard_digest) applies the filter and pre-passes its own residues."""
    from dbindex_amd import _native, shard
    pp = fasta.config("1k").slice(0, 500)
    prm = DBIndexSearchParams.trypsin(2)
    cp = prm.to_c()
    oix, n_drop, n_valid, _, _ = _expect(cp, pp, filt)
    d_res = _native.DeviceBuffer.from_numpy(np.concatenate([pp.residues, np.zeros(16, np.uint8)]), 0)
    d_off = _native.DeviceBuffer.from_numpy(pp.offsets.astype(np.uint64), 0)
    engines = [Engine(cp, 0) for _ in range(3)]
    try:
        for rep in ("cold", "warm"):
            shard.build_sharded_local(engines, d_res.ptr, pp.n_residues, d_off.ptr, pp.n_proteins,
                                      shard.protein_ranges(pp.offsets, 3), peptide_filter=make_filter(filt))
            g = shard.concat_exports([e.export() for e in engines])
            o = oix.unique()
            sts = [shard.shard_stats(e) for e in engines]
            assert sum(s.n_total for s in sts) == n_valid and sum(s.n_dropped for s in sts) == n_drop
            assert sum(s.n_unique for s in sts) == oix.n_unique, rep
            assert np.array_equal(g["mass"].view(np.uint64), o["mass"].view(np.uint64)), rep
            for k in ("prot_id", "offset", "length", "occ_off", "occ_prot"):
                assert np.array_equal(g[k].astype(np.uint64), o[k].astype(np.uint64)), (rep, k)
    finally:
        for e in engines:
            e.close()


def test_filter_changed_and_removed_between_rebuilds(Engine):
    """Warm rebuild under a filter, another filter, then none: each index is
    its own oracle's; the last is the plain index (nothing of a filter stays
    behind in the flags table, the routing or the cut-stepping count)."""
    from dbindex_amd._native import DeviceBuffer
    prm = DBIndexSearchParams.trypsin(2)
    pp = fasta.config("1k").slice(0, 300)
    cp = prm.to_c()
    plain = cref.Index(cp, pp.residues, pp.offsets)
    with Engine(cp) as eng:
        eng.build(pp)
        assert_index_equal(eng, plain, "before any filter")
        for filt in (FILTERS[1], FILTERS[1], FILTERS[2], ("C", 0)):
            oix, n_drop, _, _, _ = _expect(cp, pp, filt)
            eng.set_peptide_filter(make_filter(filt))
            with pytest.raises(Exception):
                eng.export()  # the index built under the previous setting no longer answers
            eng.rebuild()
            _assert_filtered(eng, oix, n_drop, f"rebuild under {filt}")
            eng.rebuild()
            _assert_filtered(eng, oix, n_drop, f"warm rebuild under {filt}")
        eng.set_peptide_filter(None)
        eng.rebuild()
        assert_index_equal(eng, plain, "filter removed")
        d_res = DeviceBuffer.from_numpy(np.concatenate([pp.residues, np.zeros(16, np.uint8)]))
        d_off = DeviceBuffer.from_numpy(pp.offsets.astype(np.uint64))
        assert eng.count_device(d_res.ptr, pp.n_residues, d_off.ptr, pp.n_proteins) == \
            cref.count(cp, pp.residues, pp.offsets)


# ------------------------------------------------------------- persistence
def test_filtered_index_persistence(Engine, tmp_path):
    from dbindex_amd import _native
    prm = DBIndexSearchParams.trypsin(2)
    pp = fasta.config("1k").slice(0, 300)
    cp = prm.to_c()
    filt, other = FILTERS[3], FILTERS[1]
    oix, n_drop, _, _, _ = _expect(cp, pp, filt)
    path, plain_path = str(tmp_path / "filtered.dbihip"), str(tmp_path / "plain.dbihip")

    def matches(pth, f=None):
        v = ctypes.c_int(-1)
        c = make_filter(f).to_c() if f is not None else None
        _native.check(_native.lib().dbi_index_file_matches_filtered(
            ctypes.byref(cp), ctypes.byref(c) if c is not None else None, pth.encode(), ctypes.byref(v)))
        if f is None:  # the unfiltered entry point answers the same
            w = ctypes.c_int(-1)
            _native.check(_native.lib().dbi_index_file_matches(ctypes.byref(cp), pth.encode(), ctypes.byref(w)))
            assert w.value == v.value
        return v.value

    with Engine(cp, peptide_filter=make_filter(filt)) as a:
        a.build(pp)
        a.save(path)
    with Engine(cp) as p:
        p.build(pp)
        p.save(plain_path)
    assert matches(path, filt) == 1 and matches(path, other) == 0 and matches(path) == 0
    assert matches(plain_path) == 1 and matches(plain_path, filt) == 0
    with Engine(cp, peptide_filter=make_filter(filt)) as b:
        b.load(path)
        _assert_filtered(b, oix, n_drop, "loaded under the same filter")
        with pytest.raises(_native.DBIndexStoreException):
            b.load(plain_path)
    for f in (other, None):
        with Engine(cp, peptide_filter=make_filter(f) if f is not None else None) as c:
            with pytest.raises(_native.DBIndexStoreException, match="peptide filter"):
                c.load(path)
    with Engine(cp) as e:  # an unfiltered file of this build on an unfiltered handle
        e.load(plain_path)
        assert_index_equal(e, cref.Index(cp, pp.residues, pp.offsets), "plain loaded")
    # the header word of an unfiltered file is the zero pad word it always was
    hd = open(plain_path, "rb").read(128)
    assert hd[88:128] == bytes(40)


def test_store_reuses_a_persisted_index_only_under_its_filter(tmp_path):
    from dbindex_amd import _native
    from dbindex_amd.indexer import DBIndexer, IndexerMode
    from dbindex_amd.store import DBIndexStoreHip
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")
    pp = fasta.config("1k").slice(0, 120)
    name = str(tmp_path / "db.fasta")
    f1, f2 = make_filter(FILTERS[1]), make_filter(FILTERS[2])

    def indexer(f):
        prm = DBIndexSearchParams.trypsin(2, peptide_filter=f)
        ix = DBIndexer(prm, IndexerMode.INDEX, DBIndexStoreHip(prm, persist=True), database_name=name)
        ix.init()
        return ix

    a = indexer(f1)
    assert not a.indexStore.indexExists()
    a.run(pp)
    n1 = a.indexStore.getTotalSeqCount()
    assert indexer(f1).indexStore.indexExists()       # indexExists(): found under the same filter
    assert not indexer(f2).indexStore.indexExists()   # another filter, or none: not this index
    assert not indexer(None).indexStore.indexExists()
    oix, n_drop, n_valid, _, _ = _expect(DBIndexSearchParams.trypsin(2).to_c(), pp, FILTERS[1])
    assert n1 == n_valid


# ----------------------------------------------------------- Python mirror
@pytest.mark.parametrize("filt", [FILTERS[1], FILTERS[2]], ids=[FILTER_IDS[1], FILTER_IDS[2]])
def test_indexer_modes_return_filtered_sequences(filt):
    """DBIndexer(sparam with peptide_filter): INDEX mode's getSequences and
    SEARCH_UNINDEXED's cutAndSearch (resident and streaming) return the valid
    peptides of the range, and only those."""
    from dbindex_amd import _native
    from dbindex_amd.indexer import DBIndexer, IndexerMode
    from dbindex_amd.store import MassRange, MassRangeFilteringIndexHip
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the gpu tests need an MI355X")
    pp = fasta.config("1k").slice(0, 150)
    seqs = pp.sequences()
    prm = DBIndexSearchParams.trypsin(2, peptide_filter=make_filter(filt))
    cp = prm.to_c()
    oix, _, _, d, valid = _expect(cp, pp, filt)
    u = oix.unique()
    everything = {seqs[p][o:o + n]: float(mm) for mm, p, o, n in
                  zip(d.mass.tolist(), d.pid.tolist(), d.offset.tolist(), d.length.tolist())}
    ranges = [(1500.0, 40.0), (2500.3, 2.0), (float(u["mass"][len(u["mass"]) // 2]), 0.0)]

    def want(m, t):
        return sorted(s for s, mm in everything.items() if m - t <= mm <= m + t and is_valid(filt, s))

    assert all(want(m, t) for m, t in ranges)
    assert any(len(want(m, t)) < sum(m - t <= mm <= m + t for mm in everything.values()) for m, t in ranges)
    ix = DBIndexer(prm)
    ix.init()
    ix.run(pp)
    assert ix.indexStore.getTotalSeqCount() == int(valid.sum())
    for m, t in ranges:
        got = sorted(s.getSequence() for s in ix.getSequencesUsingDaltonTolerance(m, t))
        rows = oix.query(m, t)  # getSequences(m, tol) of the bucketed store
        assert got == sorted(seqs[int(u["prot_id"][i])][int(u["offset"][i]):int(u["offset"][i]) + int(u["length"][i])]
                             for i in rows), (m, t)
        assert set(got) <= set(want(m, t)) and got, (m, t)
    for mode in (MassRangeFilteringIndexHip.RESIDENT, MassRangeFilteringIndexHip.STREAM):
        ux = DBIndexer(prm, IndexerMode.SEARCH_UNINDEXED, MassRangeFilteringIndexHip(prm, mode=mode))
        ux.init()
        ux.run(pp)
        for m, t in ranges:
            got = sorted(s.getSequence() for s in ux.getSequences([MassRange(m, t)]))
            assert got == want(m, t), (mode, m, t)
