"""CPU: the peptide filters of DBIndexer.cutSeq (DBIndexer.java:309-313;
util/PeptideFilterByMaxOccurrencies.java, util/PeptideFilterBySequence.java).

isValid is restated here (``str.count``, ``re.search``) and never taken from
the code under test.  Both filters are monotone -- once a prefix of a walk is
invalid every longer one is -- so a filtered digest is the unfiltered digest
without the occurrences whose peptide string is invalid; the first test pins
that against a literal restatement of the cutSeq loop with the filter inside
it, and tests/test_peptide_filter_gpu.py builds its expected indexes from it.

Run:  python -m pytest tests/test_peptide_filter.py -m "not gpu" -q
"""
from __future__ import annotations

import ctypes
import re

import numpy as np
import pytest

from dbindex_amd import _native, fasta
from dbindex_amd.params import (DBIndexSearchParams, DbiPeptideFilter, PeptideFilterByMaxOccurrences,
                                PeptideFilterBySequence)
from oracle import cref

# (aa, numMax) or a pattern of the accepted subset
FILTERS = [("M", 0), ("C", 1), "N[^P][ST]", "DP|KK|[RK]P.G"]
FILTER_IDS = ["M0", "C1", "NxST", "DP_KK_RKPxG"]


def is_valid(filt, s: str) -> bool:
    """isValid(peptide), restated."""
    if isinstance(filt, tuple):
        aa, num_max = filt
        return s.count(aa) <= max(num_max, 0)
    return re.search(filt, s) is None


def make_filter(filt):
    return PeptideFilterByMaxOccurrences(*filt) if isinstance(filt, tuple) else PeptideFilterBySequence(filt)


def strip_formulas(seq: str) -> str:
    """The protein as the walks see it: inline '[formula]' PTMs removed (DBIndexer.java:298)."""
    return re.sub(r"\[[^\]]*\]", "", seq)


def valid_mask(filt, d, seqs) -> np.ndarray:
    """Per occurrence of the digest d: is its peptide string -- the stripped
    protein's residues at (offset, length) -- valid."""
    stripped = [strip_formulas(s) for s in seqs]
    return np.array([is_valid(filt, stripped[p][o:o + n]) for p, o, n in
                     zip(d.pid.tolist(), d.offset.tolist(), d.length.tolist())], bool)


def filtered_oracle(cp, pp, filt, seqs=None):
    """(index of the valid, undropped occurrences; valid bucket drops; valid
    occurrences; unfiltered unique count) from the unfiltered oracle digest."""
    d = cref.digest(cp, pp.residues, pp.offsets)
    valid = valid_mask(filt, d, seqs if seqs is not None else pp.sequences())
    dropped = d.dropped.astype(bool)
    keep = valid & ~dropped
    oix = cref.Index(cp, pp.residues, pp.offsets,
                     occurrences=(d.mass[keep], d.pid[keep], d.offset[keep], d.length[keep]))
    return oix, int((valid & dropped).sum()), int(valid.sum()), d, valid


# ---------------------------------------------------------------------------
# DBIndexer.java:256-397, literally, with the filter at :310 (inputs without
# inline formulas: the '[' branch :288-303 is not taken)
# ---------------------------------------------------------------------------
def _check_cleavage(prm, seq, start, end):
    n_ok = start == 0 or (seq[start - 1] in prm.enzyme_residues and seq[start] not in prm.enzyme_nocut_residues)
    c_ok = end == len(seq) - 1 or (seq[end] in prm.enzyme_residues and seq[end + 1] not in prm.enzyme_nocut_residues)
    return (n_ok or c_ok) if prm.semi_cleavage else (n_ok and c_ok)


def _filter_sequence(prm, mass, pep):  # DBIndexStoreSQLiteMult.filterSequence :245-268
    mand = prm.mandatory_internal_aas
    if mand:
        return any(aa in pep[:-1] for aa in mand)
    return not (prm.max_precursor_mass < mass or prm.min_precursor_mass > mass)


class _UnknownElement(Exception):
    pass


def cut_seq_filtered(prm, filt, prot_seq, pid, out):
    """Appends (mass, pid, start, curSeqI) of every INCLUDE'd peptide, bucket drops included."""
    from oracle.pyref import formula_mass
    length = len(prot_seq)
    try:
        start = 0
        while start < length:
            end = start
            prec = 0.0
            if prm.h2o_plus_proton_added:
                prec += prm.h2o_proton
            prec += prm.cterm
            prec += prm.nterm
            pep_size = 0
            pep = ""
            mc = -1
            while prec <= prm.max_precursor_mass and end < length:
                pep_size += 1
                cur = prot_seq[end]
                if cur == "[":  # :288-303
                    close = prot_seq.index("]", end)
                    formula = prot_seq[end + 1:close]
                    aa_mass = formula_mass(formula)
                    if aa_mass != aa_mass:
                        raise _UnknownElement(formula)  # caught below: the rest of the protein is skipped (:400-403)
                    prot_seq = prot_seq.replace("[" + formula + "]", "")
                    end = close - (len(formula) + 2)
                    length = len(prot_seq)
                else:
                    pep += cur
                    aa_mass = prm.residue_mass.get(cur, 0.0)
                prec = prec + aa_mass
                if filt is not None and not is_valid(filt, pep):  # :310-313
                    break
                if prot_seq[end] in prm.enzyme_residues:
                    mc += 1
                if _check_cleavage(prm, prot_seq, start, end):
                    if mc > prm.max_missed_cleavages:
                        break
                    if prec > prm.max_precursor_mass:
                        break
                    if pep_size >= prm.min_pep_length and prec >= prm.min_precursor_mass:
                        if prm.mandatory_internal_aas is not None:
                            if not any(aa in pep for aa in prm.mandatory_internal_aas):
                                break
                        if _filter_sequence(prm, prec, pep):
                            out.append((prec, pid, start, len(pep)))
                end += 1
            start += 1
    except _UnknownElement:
        pass


def literal_filtered_index(prm, filt, pp, seqs):
    """The index of the literal loop's occurrences (bucket drops apart):
    (oracle index, drops, occurrences)."""
    cp = prm.to_c()
    occ = []
    for pid, s in enumerate(seqs):
        cut_seq_filtered(prm, filt, s, pid, occ)
    m = np.array([x[0] for x in occ], np.float64)
    br = 8000 // prm.index_factor
    dropped = (m.astype(np.int64) // br) > prm.index_factor - 1
    keep = ~dropped
    cols = [np.array([x[k] for x in occ], np.uint32)[keep] for k in (1, 2, 3)]
    oix = cref.Index(cp, pp.residues, pp.offsets, occurrences=(m[keep], *cols))
    return oix, int(dropped.sum()), len(occ)


CONFIGS = [
    ("full", DBIndexSearchParams.trypsin(2)),
    ("semi", DBIndexSearchParams.semi_tryptic(1)),
    ("mandK", DBIndexSearchParams.trypsin(2, mandatory_internal_aas="K")),
]


@pytest.mark.parametrize("filt", FILTERS, ids=FILTER_IDS)
@pytest.mark.parametrize("name,prm", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_filter_inside_the_walk_equals_the_post_filtered_digest(name, prm, filt):
    """Consequence 2: the loop with the filter in it (a break at the first
    invalid prefix) emits exactly the unfiltered digest's occurrences whose
    peptide string is valid, in the same order."""
    pp = fasta.config("1k").slice(0, 50)
    seqs = pp.sequences()
    lit = []
    for pid, s in enumerate(seqs):
        cut_seq_filtered(prm, filt, s, pid, lit)
    d = cref.digest(prm.to_c(), pp.residues, pp.offsets)
    valid = valid_mask(filt, d, seqs)
    assert 0 < valid.sum() < valid.shape[0], "vacuous case"
    assert len(lit) == int(valid.sum())
    m = np.array([x[0] for x in lit], np.float64)
    assert np.array_equal(m.view(np.uint64), d.mass[valid].view(np.uint64))
    for k, arr in ((1, d.pid), (2, d.offset), (3, d.length)):
        assert np.array_equal(np.array([x[k] for x in lit], np.uint32), arr[valid])
    if filt == FILTERS[0]:  # and the loop without a filter is the oracle's digest
        plain = []
        for pid, s in enumerate(seqs):
            cut_seq_filtered(prm, None, s, pid, plain)
        assert np.array_equal(np.array([x[0] for x in plain], np.float64).view(np.uint64), d.mass.view(np.uint64))


def with_formulas(seqs):
    """Inline '[formula]' PTMs in two of every three proteins, one of them
    inside a would-be motif (N[HPO3]GS strips to NGS), one of an unknown element."""
    out = []
    for i, s in enumerate(seqs):
        if i % 3 == 0 and len(s) > 40:
            s = s[:9] + "[O]" + s[9:20] + "N[HPO3]GS" + s[20:33] + ("[Qx2]" if i % 2 else "[H2O]") + s[33:]
        elif i % 3 == 1 and len(s) > 40:
            s = s[:15] + "C[H2]C" + s[15:]
        out.append(s)
    return out


@pytest.mark.parametrize("name,prm", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_literal_loop_with_formulas_is_the_oracle_digest(name, prm):
    """The restated loop's '[formula]' branch (:288-303), unfiltered, against
    the oracle's digest: the expected indexes of the filtered PTM builds
    (tests/test_peptide_filter_gpu.py) come from this loop with the filter in
    it.  Consequence 2 does NOT carry over to formula-bearing proteins: a walk
    the filter ends early no longer reaches the formulas behind it, so a later
    start consumes them instead (other masses), and an unknown element ends
    the protein later or not at all.  45 proteins, trypsin(2), filter ("M", 0):
    the literal loop keeps occurrences the post-filtered unfiltered digest does
    not have (asserted below)."""
    pp0 = fasta.config("1k").slice(0, 45)
    seqs = with_formulas(pp0.sequences())
    pp = fasta.PackedProteins.from_sequences(seqs, [fasta.uniprot_header(i) for i in range(len(seqs))])
    lit = []
    for pid, s in enumerate(seqs):
        cut_seq_filtered(prm, None, s, pid, lit)
    d = cref.digest(prm.to_c(), pp.residues, pp.offsets)
    assert len(lit) == d.mass.shape[0] > 500
    assert np.array_equal(np.array([x[0] for x in lit], np.float64).view(np.uint64), d.mass.view(np.uint64))
    for k, arr in ((1, d.pid), (2, d.offset), (3, d.length)):
        assert np.array_equal(np.array([x[k] for x in lit], np.uint32), arr)
    if name == "full":
        filt = ("M", 0)
        inside = []
        for pid, s in enumerate(seqs):
            cut_seq_filtered(prm, filt, s, pid, inside)
        post = int(valid_mask(filt, d, seqs).sum())
        assert len(inside) > post, (len(inside), post)


def _native_valid(c: DbiPeptideFilter, s: str) -> bool:
    b = s.encode("ascii")
    v = ctypes.c_int(-1)
    _native.check(_native.lib().dbi_peptide_filter_is_valid(ctypes.byref(c), b, len(b), ctypes.byref(v)))
    assert v.value in (0, 1)
    return bool(v.value)


PATTERNS = ["N[^P][ST]", "DP|KK|[RK]P.G", "K", "[A-C]..[^A-Y]", "ACDEFGHIKLMNPQRS|W|.Y", "[KR][KR]|M.M|C"]


@pytest.mark.parametrize("pat", PATTERNS)
def test_compiled_matcher_against_re(pat):
    """dbi_peptide_filter_is_valid (the compiled class masks the device
    pre-pass reads) against re.search on random strings, short ones and
    strings that hold a match at their very start or end."""
    rng = np.random.default_rng(17)
    c = PeptideFilterBySequence(pat).to_c()
    letters = list("ACDEFGHIKLMNPQRSTVWYZ")
    n_inv = 0
    for i in range(3000):
        s = "".join(rng.choice(letters, int(rng.integers(0, 40 if i % 3 else 6))))
        want = re.search(pat, s) is None
        n_inv += not want
        assert _native_valid(c, s) == want, (pat, s)
        if i < 20:
            assert PeptideFilterBySequence(pat).is_valid(s) == want
    assert 0 < n_inv < 3000


REJECTED = [
    ("A*", "quantifier"), ("A+K", "quantifier"), ("AK?", "quantifier"), ("A{2}", "quantifier"),
    ("(AK)", "group"), ("A(K|R)", "group"), ("^AK", "anchor"), ("AK$", "anchor"),
    ("\\d", "escape"), ("A\\.K", "escape"), ("[A\\]]", "escape"), ("A||K", "empty alternative"),
    ("|AK", "empty alternative"), ("AK|", "empty alternative"), ("", "empty alternative"),
    ("A|C|D|E|F|G|H|I|K", "8 alternatives"), ("A" * 17, "16 atoms"), ("[AK", "']'"), ("[]", "empty class"),
    ("[A[K]]", "nested"), ("AK]", "']'"),
]


@pytest.mark.parametrize("pat,word", REJECTED, ids=[repr(r[0][:12]) for r in REJECTED])
def test_rejected_constructs(pat, word):
    """Outside the subset: DBI_E_INVALID with a message naming the construct,
    from every entry point that takes a filter without a device."""
    c = DbiPeptideFilter(kind=2, num_max=0)
    c.spec = pat.encode()
    v = ctypes.c_int(-1)
    rc = _native.lib().dbi_peptide_filter_is_valid(ctypes.byref(c), b"AK", 2, ctypes.byref(v))
    assert rc == _native.DBI_E_INVALID
    assert word in _native.last_error(), _native.last_error()
    with pytest.raises(ValueError, match=re.escape(word)):
        PeptideFilterBySequence(pat).to_c()
    cp = DBIndexSearchParams.trypsin(2).to_c()
    m = ctypes.c_int(-1)
    assert _native.lib().dbi_index_file_matches_filtered(ctypes.byref(cp), ctypes.byref(c), b"/nonexistent",
                                                         ctypes.byref(m)) == _native.DBI_E_INVALID
    s = ctypes.c_void_p()
    _native.check(_native.lib().dbi_store_create(ctypes.byref(cp), 0, ctypes.byref(s)))
    try:
        assert _native.lib().dbi_store_set_peptide_filter(s, ctypes.byref(c)) == _native.DBI_E_INVALID
        assert word in _native.last_error()
    finally:
        _native.lib().dbi_store_close(s)


def test_rejected_overlong_pattern_and_bad_kinds():
    c = DbiPeptideFilter(kind=2, num_max=0)
    ctypes.memset(ctypes.byref(c, DbiPeptideFilter.spec.offset), ord("A"), 120)  # no terminating NUL
    v = ctypes.c_int(-1)
    L = _native.lib()
    assert L.dbi_peptide_filter_is_valid(ctypes.byref(c), b"AK", 2, ctypes.byref(v)) == _native.DBI_E_INVALID
    assert "119" in _native.last_error()
    with pytest.raises(ValueError, match="119"):
        PeptideFilterBySequence("AC" * 60).to_c()
    bad = DbiPeptideFilter(kind=3, num_max=0)
    assert L.dbi_peptide_filter_is_valid(ctypes.byref(bad), b"AK", 2, ctypes.byref(v)) == _native.DBI_E_INVALID
    noaa = DbiPeptideFilter(kind=1, num_max=2)
    assert L.dbi_peptide_filter_is_valid(ctypes.byref(noaa), b"AK", 2, ctypes.byref(v)) == _native.DBI_E_INVALID
    # the longest pattern that fits is accepted
    ok = PeptideFilterBySequence("|".join(["ACDEFGHIKLMNPQ"] * 8)[:119])
    assert ok.is_valid("ACDEFGHIKLMNP") and not ok.is_valid("WACDEFGHIKLMNPQW")


def test_max_occurrences_and_negative_num_max():
    """numMax < 0 behaves as 0 (numMatches > numMax at the first aa either way)."""
    rng = np.random.default_rng(3)
    for num_max in (-1, 0, 1, 2, 5):
        f = PeptideFilterByMaxOccurrences("C", num_max)
        c = f.to_c()
        for _ in range(400):
            s = "".join(rng.choice(list("ACCK"), int(rng.integers(0, 12))))
            want = s.count("C") <= max(num_max, 0)
            assert _native_valid(c, s) == want == f.is_valid(s), (num_max, s)
    a, b = PeptideFilterByMaxOccurrences("C", -1).to_c(), PeptideFilterByMaxOccurrences("C", 0).to_c()
    for s in ("", "AAAK", "C", "ACA", "CC"):
        assert _native_valid(a, s) == _native_valid(b, s)


def test_python_mirror_of_the_filters():
    """__str__ is the Java toString (the ", pepFilter:" part of the params
    string, IndexUtil.java:295-296); None and kind 0 mean no filter."""
    assert str(PeptideFilterByMaxOccurrences("C", 2)) == "C2"
    assert str(PeptideFilterByMaxOccurrences("CM", 2)) == "C2"  # aa.toCharArray()[0]
    assert str(PeptideFilterBySequence("N[^P][ST]")) == "N[^P][ST]"
    assert DBIndexSearchParams.trypsin(2).peptide_filter is None
    prm = DBIndexSearchParams.trypsin(2, peptide_filter=PeptideFilterByMaxOccurrences("C", 2))
    plain = DBIndexSearchParams.trypsin(2)
    assert bytes(prm.to_c()) == bytes(plain.to_c())  # dbi_params is unchanged
    v = ctypes.c_int(-1)
    _native.check(_native.lib().dbi_peptide_filter_is_valid(None, b"CCCC", 4, ctypes.byref(v)))
    assert v.value == 1
    none = DbiPeptideFilter(kind=0)
    _native.check(_native.lib().dbi_peptide_filter_is_valid(ctypes.byref(none), b"CCCC", 4, ctypes.byref(v)))
    assert v.value == 1
