// dbi_filter.cpp — the peptide filters of DBIndexer.cutSeq (DBIndexer.java:
// 309-313) on the host: validation, the compiled form of a sequence motif and
// isValid over it.  The reference ships two filters:
//   PeptideFilterByMaxOccurrencies(aa, numMax)   util/PeptideFilterByMaxOccurrencies.java
//   PeptideFilterBySequence(regexp)              util/PeptideFilterBySequence.java
// java.util.regex is not reimplemented: a pattern is accepted only where
// Matcher.find is a plain motif search (alternatives of fixed-length class
// sequences); anything else is rejected by name, never ignored.
#include <cstring>
#include <string>

#include "dbi_internal.h"

namespace dbi {

namespace {

int reject(const std::string& what, size_t at) {
    return set_error(DBI_E_INVALID, "peptide filter pattern: " + what + " at character " + std::to_string(at) +
                                        " is outside the supported subset (alternatives of literals, '.' and "
                                        "[...] classes)");
}

void set_bit(uint32_t* m, unsigned c) { m[c >> 5] |= 1u << (c & 31); }

// one [...] class starting after '['; returns the index after ']' or 0 on error (error set)
size_t parse_class(const char* p, size_t n, size_t i, uint32_t* m, int* rc) {
    bool neg = false;
    if (i < n && p[i] == '^') {
        neg = true;
        ++i;
    }
    uint32_t cls[8] = {};
    size_t members = 0;
    for (;;) {
        if (i >= n) {
            *rc = reject("a '[' without ']'", i);
            return 0;
        }
        const unsigned char c = (unsigned char)p[i];
        if (c == ']') {
            if (members == 0) {
                *rc = reject("an empty class", i);
                return 0;
            }
            ++i;
            break;
        }
        if (c == '\\') {
            *rc = reject("an escape ('\\')", i);
            return 0;
        }
        if (c == '[' || c == '&') {  // Java: nested classes, && intersections
            *rc = reject(c == '[' ? "a nested class" : "a class intersection ('&')", i);
            return 0;
        }
        if (c == '^') {
            *rc = reject("a '^' inside a class", i);
            return 0;
        }
        if (c == '-') {
            *rc = reject("a '-' that is not between two class members", i);
            return 0;
        }
        if (i + 2 < n && p[i + 1] == '-' && p[i + 2] != ']') {
            const unsigned char d = (unsigned char)p[i + 2];
            if (d == '\\' || d == '[' || d == '^' || d == '-' || d == '&' || d < c) {
                *rc = reject("a malformed range", i);
                return 0;
            }
            for (unsigned x = c; x <= d; ++x) set_bit(cls, x);
            i += 3;
        } else if (i + 1 < n && p[i + 1] == '-') {
            *rc = reject("a '-' that is not between two class members", i + 1);
            return 0;
        } else {
            set_bit(cls, c);
            ++i;
        }
        ++members;
    }
    for (int w = 0; w < 8; ++w) m[w] = neg ? ~cls[w] : cls[w];
    return i;
}

}  // namespace

int pf_compile(const dbi_peptide_filter* f, PepFilterProg* prog) {
    std::memset(prog, 0, sizeof(*prog));
    if (!f || f->kind == 0) return 0;
    if (f->kind == 1) {
        if (f->spec[0] == 0) return set_error(DBI_E_INVALID, "peptide filter: max occurrences needs a residue (spec[0])");
        return 0;
    }
    if (f->kind != 2) return set_error(DBI_E_INVALID, "peptide filter: unknown kind (0 none, 1 max occurrences, 2 motif)");
    const size_t n = strnlen(f->spec, sizeof(f->spec));
    if (n == sizeof(f->spec))
        return set_error(DBI_E_INVALID, "peptide filter pattern: more than 119 characters (or no terminating NUL)");
    if (n == 0) return set_error(DBI_E_INVALID, "peptide filter pattern: an empty alternative (the empty pattern)");
    const char* p = f->spec;
    uint32_t a = 0, k = 0;
    for (size_t i = 0; i < n;) {
        const unsigned char c = (unsigned char)p[i];
        if (c == '|') {
            if (k == 0) return reject("an empty alternative", i);
            prog->len[a++] = k;
            k = 0;
            if (a >= (uint32_t)PF_MAX_ALTS) return reject("more than 8 alternatives", i);
            ++i;
            continue;
        }
        const char* bad = nullptr;
        switch (c) {
        case '*': case '+': case '?': case '{': case '}': bad = "a quantifier"; break;
        case '(': case ')': bad = "a group"; break;
        case '^': case '$': bad = "an anchor"; break;
        case '\\': bad = "an escape ('\\')"; break;
        case ']': bad = "a ']' without '['"; break;
        default: break;
        }
        if (bad) return reject(bad, i);
        if (k >= (uint32_t)PF_MAX_ATOMS) return reject("an alternative of more than 16 atoms", i);
        uint32_t* m = prog->mask[a][k];
        if (c == '.') {
            for (int w = 0; w < 8; ++w) m[w] = ~0u;
            m['\n' >> 5] &= ~(1u << ('\n' & 31));  // Java's '.' excludes line terminators
            m['\r' >> 5] &= ~(1u << ('\r' & 31));
            m[0x85 >> 5] &= ~(1u << (0x85 & 31));
            ++i;
        } else if (c == '[') {
            int rc = 0;
            i = parse_class(p, n, i + 1, m, &rc);
            if (rc) return rc;
        } else {
            set_bit(m, c);
            ++i;
        }
        ++k;
    }
    if (k == 0) return reject("an empty alternative", n);
    prog->len[a++] = k;
    prog->n_alt = a;
    return 0;
}

bool pf_is_valid(const dbi_peptide_filter& f, const PepFilterProg& prog, const uint8_t* seq, uint64_t len) {
    if (f.kind == 1) {
        const int64_t lim = f.num_max < 0 ? 0 : f.num_max;
        int64_t cnt = 0;
        for (uint64_t i = 0; i < len; ++i)
            if (seq[i] == (uint8_t)f.spec[0] && ++cnt > lim) return false;
        return true;
    }
    if (f.kind != 2) return true;
    for (uint64_t e = 0; e < len; ++e)  // a match ending at e
        for (uint32_t a = 0; a < prog.n_alt; ++a) {
            const uint32_t L = prog.len[a];
            if (L > e + 1) continue;
            bool ok = true;
            for (uint32_t k = 0; k < L && ok; ++k) {
                const uint8_t c = seq[e + 1 - L + k];
                ok = (prog.mask[a][k][c >> 5] >> (c & 31)) & 1u;
            }
            if (ok) return false;
        }
    return true;
}

uint64_t pf_hash(const dbi_peptide_filter* f) {
    if (!f || f->kind == 0) return 0;
    uint64_t h = 0xcbf29ce484222325ull;
    auto mix = [&h](const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    };
    const int32_t kind = f->kind, num_max = f->kind == 1 ? f->num_max : 0;
    mix(&kind, 4);
    mix(&num_max, 4);
    mix(f->spec, f->kind == 1 ? 1 : strnlen(f->spec, sizeof(f->spec)));
    return h ? h : 1;
}

}  // namespace dbi

extern "C" int dbi_peptide_filter_is_valid(const dbi_peptide_filter* f, const char* seq, uint64_t len, int* out) {
    using namespace dbi;
    if (!out || (!seq && len)) return set_error(DBI_E_INVALID, "NULL argument");
    PepFilterProg prog;
    const int rc = pf_compile(f, &prog);
    if (rc) return rc;
    *out = (!f || f->kind == 0) ? 1 : pf_is_valid(*f, prog, reinterpret_cast<const uint8_t*>(seq), len) ? 1 : 0;
    return 0;
}
