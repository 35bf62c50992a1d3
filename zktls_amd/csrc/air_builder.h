// air_builder.h -- how every chip of this library writes its constraint program and its interaction table: ONE definition of the term list, the variable words,
// the selectors, the two builders and the expression algebra over term lists.  A chip file includes this and says `using namespace airb;` where its builders live.
//   program (air.h):            {AIR_MAGIC, 1, width, constraints, public values, words} then per constraint {selector, terms, per term {coefficient, degree, variables...}}
//   interaction table (air.h):  {LOOKUP_MAGIC, entries, words} then per entry {sign (0 send, 1 receive), multiplicity column, bus, n, columns...}
// The ORDER in which terms and entries are added is the program: the Python restatements under tests/ add them in the same order, and the words must be equal.
#pragma once
#include <array>
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "air.h"

namespace zk {
namespace airb {

struct Term { uint32_t coeff; std::vector<uint32_t> vars; };
typedef std::vector<Term> Terms;
inline uint32_t var(uint32_t col, bool next = false) { return next ? ((1u << 30) | col) : col; }
inline uint32_t pub(uint32_t idx) { return (2u << 30) | idx; }
inline uint32_t neg(uint64_t c) { c %= P; return c ? (uint32_t)(P - c) : 0u; }
inline uint32_t mulm(uint64_t a, uint64_t b) { return (uint32_t)((a % P) * (b % P) % P); }
enum : uint32_t { ALL = 0, FIRST = 1, LAST = 2, TRANSITION = 3 };

// `body` and `count` are open: a chip may start from constraints written elsewhere (p2chip::permutation_body hands a body and its count over)
struct Builder {
    std::vector<uint32_t> body;
    uint32_t count = 0;
    void add(uint32_t selector, const Terms& terms) {          // coefficients are reduced; terms with coefficient 0 are omitted
        body.push_back(selector);
        const size_t at = body.size();
        body.push_back(0u);
        uint32_t kept = 0;
        for (const Term& t : terms) {
            if (t.coeff % P == 0) continue;
            body.push_back(t.coeff % P);
            body.push_back((uint32_t)t.vars.size());
            for (uint32_t v : t.vars) body.push_back(v);
            kept++;
        }
        body[at] = kept;
        count++;
    }
    std::vector<uint32_t> finish(uint32_t width, uint32_t n_public) const {
        std::vector<uint32_t> p{AIR_MAGIC, 1u, width, count, n_public, (uint32_t)(6 + body.size())};
        p.insert(p.end(), body.begin(), body.end());
        return p;
    }
};

// ---- polynomials over columns: a list of (coefficient, variables); an extension expression = four of them (x^4 = 11).  No merging of
// like terms: the order in which terms are produced IS the program (tests/recursion_air.py's helpers produce them in the same order).
typedef std::array<Terms, 4> EE;
inline Terms pc(uint64_t c) { c %= P; return c ? Terms{Term{(uint32_t)c, {}}} : Terms{}; }
inline Terms pv(uint32_t col, bool nxt = false) { return Terms{Term{1u, {var(col, nxt)}}}; }
inline Terms ppub(uint32_t i) { return Terms{Term{1u, {pub(i)}}}; }
inline Terms padd(const Terms& a, const Terms& b) { Terms o = a; o.insert(o.end(), b.begin(), b.end()); return o; }
inline Terms pscale(const Terms& a, uint64_t k) { Terms o; for (const Term& t : a) { const uint32_t c = mulm(t.coeff, k); if (c) o.push_back(Term{c, t.vars}); } return o; }
inline Terms pneg(const Terms& a) { return pscale(a, P - 1); }
inline Terms pmul(const Terms& a, const Terms& b) {
    Terms o;
    for (const Term& x : a) for (const Term& y : b) { const uint32_t c = mulm(x.coeff, y.coeff); if (!c) continue; Term t{c, x.vars}; t.vars.insert(t.vars.end(), y.vars.begin(), y.vars.end()); o.push_back(t); }
    return o;
}
inline EE ev(uint32_t col, bool nxt = false) { return EE{pv(col, nxt), pv(col + 1, nxt), pv(col + 2, nxt), pv(col + 3, nxt)}; }
inline EE ec(uint64_t c0, uint64_t c1 = 0, uint64_t c2 = 0, uint64_t c3 = 0) { return EE{pc(c0), pc(c1), pc(c2), pc(c3)}; }
inline EE eb(const Terms& p) { return EE{p, Terms{}, Terms{}, Terms{}}; }
inline EE epub(uint32_t idx) { return EE{ppub(idx), ppub(idx + 1), ppub(idx + 2), ppub(idx + 3)}; }
inline EE eone() { return ec(1); }
inline EE eadd(const EE& a, const EE& b) { return EE{padd(a[0], b[0]), padd(a[1], b[1]), padd(a[2], b[2]), padd(a[3], b[3])}; }
inline EE eadd(const EE& a, const EE& b, const EE& c) { return eadd(eadd(a, b), c); }
inline EE esub(const EE& a, const EE& b) { return EE{padd(a[0], pneg(b[0])), padd(a[1], pneg(b[1])), padd(a[2], pneg(b[2])), padd(a[3], pneg(b[3]))}; }
inline EE escale(const EE& a, uint64_t k) { return EE{pscale(a[0], k), pscale(a[1], k), pscale(a[2], k), pscale(a[3], k)}; }
inline EE emul(const EE& a, const EE& b) {
    EE o;
    for (int j = 0; j < 4; j++)
        for (int i = 0; i < 4; i++)
            for (int k = 0; k < 4; k++) {
                if ((i + k) % 4 != j) continue;
                Terms t = pmul(a[i], b[k]);
                if (i + k >= 4) t = pscale(t, EXT_W);
                o[j].insert(o[j].end(), t.begin(), t.end());
            }
    return o;
}
inline EE egate(const Terms& f, const EE& e) { return EE{pmul(f, e[0]), pmul(f, e[1]), pmul(f, e[2]), pmul(f, e[3])}; }
inline void add_ext(Builder& b, uint32_t sel, const EE& e) { for (int i = 0; i < 4; i++) b.add(sel, e[i]); }

// zps_k(zeta) = a_k zeta^N + b_k, N = 2^n, for the two quotient chunks over the cosets g w_{2N}^k <w_N> (canonical): what the SCALARS chip of the shard verifier
// (shard_verifier.inl) and SCALARS16 of the fold-16 identity machine (fri16_chip.hip) put the quotient together with
inline void zps_consts(int n, uint32_t a[2], uint32_t b[2]) {
    const uint64_t N = (uint64_t)1 << n;
    const uint32_t wq = two_adic_generator(n + 1);
    uint32_t sN[2];
    for (int k = 0; k < 2; k++) sN[k] = fpow(fmul(MONTY_GEN, fpow(wq, (uint64_t)k)), N);
    for (int k = 0; k < 2; k++) {
        const int j = 1 - k;
        const uint32_t sj_inv = finv(sN[j]);
        const uint32_t den_inv = finv(fsub(fmul(sN[k], sj_inv), MONTY_R1));
        a[k] = from_monty(fmul(sj_inv, den_inv));
        b[k] = from_monty(fneg(den_inv));
    }
}

struct Interactions {
    std::vector<uint32_t> w{LOOKUP_MAGIC, 0u, 0u};
    void add(uint32_t sign, uint32_t mult, uint32_t bus, std::initializer_list<uint32_t> cols) {
        w.push_back(sign); w.push_back(mult); w.push_back(bus); w.push_back((uint32_t)cols.size());
        w.insert(w.end(), cols.begin(), cols.end());
        w[1]++; w[2] = (uint32_t)w.size();
    }
    const std::vector<uint32_t>& finish() const { return w; }
};

}  // namespace airb
}  // namespace zk
