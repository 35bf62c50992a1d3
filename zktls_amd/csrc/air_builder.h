// air_builder.h -- how every chip of this library writes its constraint program and its interaction table: ONE definition of the term list, the variable words,
// the selectors and the two builders.  A chip file includes this and says `using namespace airb;` where its builders live.
//   program (air.h):            {AIR_MAGIC, 1, width, constraints, public values, words} then per constraint {selector, terms, per term {coefficient, degree, variables...}}
//   interaction table (air.h):  {LOOKUP_MAGIC, entries, words} then per entry {sign (0 send, 1 receive), multiplicity column, bus, n, columns...}
// The ORDER in which terms and entries are added is the program: the Python restatements under tests/ add them in the same order, and the words must be equal.
#pragma once
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
