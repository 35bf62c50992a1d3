"""A catalogue of FORGED inner proofs for the recursion provers (zkhip_prove_machine_verifier and what is built on it, zkhip_prove_shard_verifier): for a
version-11 keyed-machine proof (described by recursion_machine.MShape) and for a version-1 / version-7 shard proof, the word offset of every site whose change one
check of the verifier -- and no other -- must notice, with the set of checks it breaks and the chain the device kernels walk it in.

Computed from the proof FORMAT (docs/PROTOCOL.md; the order tests/pyverify_chips.py and tests/pyverify.py take the words in), not from the library.  No GPU and no
library call in here.  A forgery is w[off] = (w[off] + 1) % P: the word stays canonical (a `^ 1` on the even word P - 1 would not, and a non-canonical word is
refused on another path).  Lengths, header and shape words are never touched, so every read of a kernel stays at its honest address.

Checks are named by the strings below; a forgery's `breaks` is the set of checks a verifier may name when it refuses it (which one it meets first depends on the
order it walks in: a moved sibling breaks its layer's opening AND the value the chain ends in).  `gid` is the chain's number as the chain kernels count it."""
import struct
from collections import namedtuple

P = 2013265921

KEY, TRACE, PERM, QUOT, FINAL, TRANSCRIPT = "key opening", "trace opening", "permutation opening", "quotient opening", "final value", "transcript"
OPENING_OF = {"E": KEY, "T": TRACE, "P": PERM, "Q": QUOT}


def LAYER(l):
    return "FRI layer %d opening" % l


# field: what the word is in the view the Python verifiers fill -- ("tpath", lvl, j), ("sibs", l, j), ("paths", l, lvl, j), ("trows", c, i), ("trace_root", j), ...
Forgery = namedtuple("Forgery", "p q kind field off breaks gid")


def words_of(proof):
    b = bytes(proof)
    return list(struct.unpack("<%dI" % (len(b) // 4), b))


def forge(proof, off):
    """-> the proof's bytes with word `off` moved by one (mod P)"""
    b = bytearray(bytes(proof))
    (v,) = struct.unpack_from("<I", b, 4 * off)
    struct.pack_into("<I", b, 4 * off, (v + 1) % P)
    return bytes(b)


def forge_many(proof, offs):
    b = bytes(proof)
    for off in offs:
        b = forge(b, off)
    return b


def _levels(depth):
    """level 0, a middle level, the top level"""
    return sorted({0, depth // 2, depth - 1})


def _row_words(n):
    """first word, last word, the words on either side of the first 8-word sponge block boundary"""
    return sorted({0, n - 1} | ({7, 8} if n > 8 else set()))


# ---------------------------------------------------------------------------------------------------------------- version 11: the keyed machine
PATH_FIELD = {"E": "epath", "T": "tpath", "P": "ppath", "Q": "qpath"}
ROW_FIELD = {"E": "erows", "T": "trows", "P": "prows", "Q": "qrows"}


class MachineLayout:
    """where the words of a version-11 proof of the machine `sh` (recursion_machine.MShape) stand"""
    def __init__(self, sh):
        self.sh = sh
        C, R, H = sh.C, sh.R, sh.H
        # magic | version, chips, blowup, queries, pow bits, publics | 16 | chip entries | program digests | table digests | the key's root: sh.head lacks the magic and the 16
        pos = sh.HL + 2
        self.troot = pos; pos += 8
        self.proot = pos; pos += 8
        self.cum = pos; pos += 4 * C                        # every chip of a machine talks to another: one cumulative sum each
        self.qroot = pos; pos += 8
        self.opened = pos; pos += 4 * sh.NV
        self.lroots = pos; pos += 8 * R
        self.final = pos; pos += 4
        self.witness = pos; pos += 1
        self.queries = pos
        # one query: per commitment (key, main, permutation, quotient) the rows of its chips in chip order, then its path; then per layer the sibling and the path
        at = 0
        self.row = {}                                       # (tree, chip) -> offset in the query
        self.path = {}                                      # tree -> offset in the query
        self.depth = {}
        for t in sh.trees:
            for c in sh.tree_chips[t]:
                self.row[(t, c)] = at
                at += sh.tree_w[t][c]
            self.path[t], self.depth[t] = at, sh.tree_hs[t][0]
            at += 8 * sh.tree_hs[t][0]
        self.sib, self.lpath = [], []
        for l in range(R):
            self.sib.append(at)
            self.lpath.append(at + 4)
            at += 4 + 8 * (H - 1 - l)
        self.per_query = at
        self.words = self.queries + sh.Q * at
        self.n_trees = len(sh.trees)
        self.per_q_chains = self.n_trees + R
        self.n_chains = sh.NP * sh.Q * self.per_q_chains

    def q_at(self, q):
        return self.queries + q * self.per_query

    def gid(self, p, q, c):
        """commitments first (key, main, permutation, quotient: those the machine has), the layers behind"""
        return (p * self.sh.Q + q) * self.per_q_chains + c

    def tree_gid(self, p, q, t):
        return self.gid(p, q, self.sh.trees.index(t))

    def layer_gid(self, p, q, l):
        return self.gid(p, q, self.n_trees + l)

    def lane(self, p, q):
        """the (proof, query) lane of the fold and row-sum kernels"""
        return p * self.sh.Q + q


def machine_query_sites(lay, p, q):
    """every per-query site of the catalogue for query q of proof p"""
    sh, out, base = lay.sh, [], lay.q_at(q)
    R = sh.R
    for t in sh.trees:                                      # a commitment's path digest: that opening only
        for lvl in _levels(lay.depth[t]):
            for j in (0, 7):
                out.append(Forgery(p, q, "commit path", (PATH_FIELD[t], lvl, j), base + lay.path[t] + 8 * lvl + j, frozenset({OPENING_OF[t]}), lay.tree_gid(p, q, t)))
    for l in sorted({0, R - 1}):                            # a layer's path digest: that layer's opening only
        for lvl in _levels(sh.H - 1 - l):
            for j in (0, 7):
                out.append(Forgery(p, q, "layer path", ("paths", l, lvl, j), base + lay.lpath[l] + 8 * lvl + j, frozenset({LAYER(l)}), lay.layer_gid(p, q, l)))
    for l in sorted({0, R - 1}):                            # a sibling: the layer's leaf, and the value the chain goes on with
        for j in (0, 3):
            out.append(Forgery(p, q, "sibling", ("sibs", l, j), base + lay.sib[l] + j, frozenset({LAYER(l), FINAL}), lay.layer_gid(p, q, l)))
    for t in sh.trees:                                      # an opened row word: the leaf (or the digest injected mid-path), the reduced opening, the chain's end
        hs = sh.tree_hs[t]
        for h in hs[:1] + hs[-1:] if len(hs) > 1 else hs:
            segs, n = sh.leaf_segs[(t, h)]
            # the reduced opening of height h joins the fold chain where the chain has come down to 2^h rows: the value layer H - h opens (layer 0 for the tallest)
            joins = frozenset({LAYER(sh.H - h)}) if sh.H - h < R else frozenset()
            for i in _row_words(n):
                c, at, w = next(s for s in segs if s[1] <= i < s[1] + s[2])
                out.append(Forgery(p, q, "row word", (ROW_FIELD[t], c, i - at), base + lay.row[(t, c)] + (i - at), frozenset({OPENING_OF[t], FINAL}) | joins, lay.tree_gid(p, q, t)))
    return out


def machine_transcript_sites(lay, p):
    """words that move the transcript: refused by the host pass under either setting, by whichever check meets the moved challenges first"""
    any_ = frozenset({TRANSCRIPT})
    return [Forgery(p, None, "transcript", ("trace_root", 3), lay.troot + 3, any_, None), Forgery(p, None, "transcript", ("quot_root", 0), lay.qroot, any_, None),
            Forgery(p, None, "transcript", ("opened", 5), lay.opened + 5, any_, None), Forgery(p, None, "transcript", ("layer_roots", 0, 7), lay.lroots + 7, any_, None),
            Forgery(p, None, "transcript", ("final", 2), lay.final + 2, any_, None)]


def machine_catalogue(sh, lanes=None):
    """-> (layout, [Forgery]) for the listed (proof, query) pairs (all of them when None) and the transcript sites of every proof"""
    lay = MachineLayout(sh)
    lanes = [(p, q) for p in range(sh.NP) for q in range(sh.Q)] if lanes is None else lanes
    out = []
    for p, q in lanes:
        out += machine_query_sites(lay, p, q)
    for p in range(sh.NP):
        out += machine_transcript_sites(lay, p)
    return lay, out


def machine_view_word(view, f):
    """the word the forgery names, out of the view tests/pyverify_chips.verify(..., view=) fills"""
    name = f.field[0]
    if f.q is None:
        if name == "opened":                                # the stream in proof order: per chip el | en | tl | tn | pl | pn | q, four words per value
            flat = [x for parts in view["opened"] for part in parts[5:] + parts[:5] for e in part for x in e]
            return flat[f.field[1]]
        v = view[name]
        for i in f.field[1:]:
            v = v[i]
        return v
    v = view["queries"][f.q][name]
    for i in f.field[1:]:
        v = v[i]
    return v


# ---------------------------------------------------------------------------------------------------------------- versions 1 and 7: the shard proof
class ShardLayout:
    """where the words of a shard proof of the default shape (blowup 2, fold by 2, a constant final value, the width-16 hash) stand; air: version 7 (a constraint
    program of degree <= 3: two quotient chunks), whose header carries four more shape words and the program's digest"""
    def __init__(self, log_n, width, n_queries, n_proofs, air=False):
        self.n, self.W, self.Q, self.NP = log_n, width, n_queries, n_proofs
        self.R, self.H = log_n, log_n + 1
        pos = 20 if air else 8
        self.troot = pos; pos += 8
        self.qroot = pos; pos += 8
        self.opened = pos; pos += 8 * width + 32            # values at zeta, at zeta g, the eight quotient columns: extension values
        self.lroots = pos; pos += 8 * self.R
        self.final = pos; pos += 4
        self.witness = pos; pos += 1
        self.queries = pos
        H = self.H
        self.trow, self.tpath, self.qrow, self.qpath = 0, width, width + 8 * H, width + 8 * H + 8
        at = width + 8 * H + 8 + 8 * H
        self.sib, self.lpath = [], []
        for l in range(self.R):
            self.sib.append(at)
            self.lpath.append(at + 4)
            at += 4 + 8 * (H - 1 - l)
        self.per_query = at
        self.words = self.queries + n_queries * at
        self.chains_per = n_queries * self.R + 2 * n_queries
        self.n_chains = n_proofs * self.chains_per

    def q_at(self, q):
        return self.queries + q * self.per_query

    # the shard verifier's chain list: per proof the layers query by query, then every query's trace opening, then every query's quotient opening
    def layer_gid(self, p, q, l):
        return p * self.chains_per + q * self.R + l

    def tree_gid(self, p, q, t):
        return p * self.chains_per + self.Q * self.R + (self.Q if t == "Q" else 0) + q


def shard_query_sites(lay, p, q):
    out, base, R, H = [], lay.q_at(q), lay.R, lay.H
    for t, path, field in (("T", lay.tpath, "tpath"), ("Q", lay.qpath, "qpath")):
        for lvl in _levels(H):
            for j in (0, 7):
                out.append(Forgery(p, q, "commit path", (field, lvl, j), base + path + 8 * lvl + j, frozenset({OPENING_OF[t]}), lay.tree_gid(p, q, t)))
    for l in sorted({0, R - 1}):
        for lvl in _levels(H - 1 - l):
            for j in (0, 7):
                out.append(Forgery(p, q, "layer path", ("paths", l, lvl, j), base + lay.lpath[l] + 8 * lvl + j, frozenset({LAYER(l)}), lay.layer_gid(p, q, l)))
    for l in sorted({0, R - 1}):
        for j in (0, 3):
            out.append(Forgery(p, q, "sibling", ("sibs", l, j), base + lay.sib[l] + j, frozenset({LAYER(l), FINAL}), lay.layer_gid(p, q, l)))
    for t, row, n, field in (("T", lay.trow, lay.W, "trow"), ("Q", lay.qrow, 8, "qrow")):
        for i in _row_words(n):
            out.append(Forgery(p, q, "row word", (field, i), base + row + i, frozenset({OPENING_OF[t], LAYER(0), FINAL}), lay.tree_gid(p, q, t)))
    return out


def shard_transcript_sites(lay, p):
    any_ = frozenset({TRANSCRIPT})
    return [Forgery(p, None, "transcript", ("trace_root", 3), lay.troot + 3, any_, None), Forgery(p, None, "transcript", ("quot_root", 0), lay.qroot, any_, None),
            Forgery(p, None, "transcript", ("loc", 1, 1), lay.opened + 5, any_, None), Forgery(p, None, "transcript", ("roots", 0, 7), lay.lroots + 7, any_, None),
            Forgery(p, None, "transcript", ("final", 2), lay.final + 2, any_, None)]


def shard_catalogue(log_n, width, n_queries, n_proofs, air=False, lanes=None):
    lay = ShardLayout(log_n, width, n_queries, n_proofs, air)
    lanes = [(p, q) for p in range(n_proofs) for q in range(n_queries)] if lanes is None else lanes
    out = []
    for p, q in lanes:
        out += shard_query_sites(lay, p, q)
    for p in range(n_proofs):
        out += shard_transcript_sites(lay, p)
    return lay, out


def shard_view_word(view, f):
    """the word the forgery names, out of the view tests/pyverify.verify(..., view=) fills"""
    name = f.field[0]
    if f.q is None:
        v = view[name]
        for i in f.field[1:]:
            v = v[i]
        return v
    if name == "sibs":
        return view["queries"][f.q][2][f.field[1]][f.field[2]]
    if name == "paths":
        return view["paths"][f.q][f.field[1]][f.field[2]][f.field[3]]
    v = view["openings"][f.q][name]
    for i in f.field[1:]:
        v = v[i]
    return v


# ---------------------------------------------------------------------------------------------------------------- what the verdicts mean
# the Python verifiers' Reject reasons -> the check (layer reasons carry the layer's number: see check_of_reject)
REJECT_REASONS = {"preprocessed opening": KEY, "trace opening": TRACE, "permutation opening": PERM, "quotient opening": QUOT, "final value": FINAL, "final polynomial": FINAL}
# the stand-alone host verifiers' reason codes (zkhip_verify_machine_keyed, zkhip_verify_shard) -> the check; 40 + l: layer l
REASON_CODES = {33: KEY, 30: TRACE, 32: PERM, 31: QUOT, 100: FINAL}
# the provers' phrases (after "proof p rejected: ") -> the checks each may stand for.  Machine mode names the class of a layer or an opening, not which one.
OPENINGS = frozenset({KEY, TRACE, PERM, QUOT})
MACHINE_PHRASES = {"a FRI layer opening does not end in the layer's root": "layers", "a fold chain does not end in the final value": frozenset({FINAL}),
                   "an opening does not end in its root": OPENINGS}
# the shard verifier, per setting.  Device witnesses: its chain kernel hands back every chain's root -- commitments and layers alike -- and the host compares: one
# phrase for both; the fold kernel's finals are compared before them.  Host witnesses: the host's verifier pass (paths not hashed) refuses a chain's end by its reason
# code, the chain kernel's roots are compared as above.
SHARD_PHRASES = {
    0: {"an opening does not end in its root": "openings and layers", "a fold chain does not end in the final value": frozenset({FINAL})},
    1: {"an opening does not end in its root": "openings and layers", "proof rejected (check 100)": frozenset({FINAL})},
}


def check_of_reject(reason):
    if reason.startswith("FRI layer ") and reason.endswith(" opening"):
        return LAYER(int(reason.split()[2]))
    return REJECT_REASONS[reason]


def check_of_code(code):
    return LAYER(code - 40) if 40 <= code <= 90 else REASON_CODES[code]


def phrase_fits(phrases, message, breaks):
    """does the phrase the prover's message ends in belong to a check of `breaks`?  -> the phrase (None: no known phrase, or one of another class).
    The provers' phrases name a CLASS (some layer, some opening), so a class fits when `breaks` holds any member of it.  Sibling and row-word entries always hold
    FINAL, which the fold kernels report: a chain kernel that never noticed a forged leaf would still pass on those.  It is the path-digest entries -- one check each,
    one chain each -- that pin the chain kernels' refusals."""
    for phrase, stands in phrases.items():
        if not message.endswith(phrase):
            continue
        if stands == "layers":
            ok = any(b.startswith("FRI layer ") for b in breaks)
        elif stands == "openings and layers":
            ok = any(b in OPENINGS or b.startswith("FRI layer ") for b in breaks)
        else:
            ok = bool(stands & breaks)
        return phrase if ok else None
    return None


def single(entries):
    """the forgeries that break exactly one check"""
    return [f for f in entries if len(f.breaks) == 1 and f.q is not None]


def thinned(entries):
    """one site of every (query, kind, chain, set of checks) -- which one moves with the query, so that the levels and words still vary over a shape's lanes"""
    groups = {}
    for f in entries:
        groups.setdefault((f.p, f.q, f.kind, f.gid, f.breaks), []).append(f)
    return [g[((k[0] or 0) + (k[1] or 0)) % len(g)] if k[1] is not None else g[0] for k, g in groups.items()]


# ---------------------------------------------------------------------------------------------------------------- the shapes the tests run on
SEED = 0x5A4B544C53
SP1_SMALL = [(8, 24, 3, 1), (8, 32, 3, 0), (7, 16, 2, -1), (6, 32, 2, -1), (5, 8, 1, -1)]
WIDE_Q = 33
# the wide shape's lanes: queries 0, 15, 16, 31, 32 of proof 0 (the host's groups of sixteen: first and last lane of a full group, the lone query of the last) and
# lanes 63, 64, 65 of the (proof, query) kernels (either side of the first workgroup of 64, and the last lane)
FIRST_AND_LAST = ((0, 0), (1, 2))                         # of two proofs of three queries: the first chain's lane and the last's
WIDE_LANES = [(0, 0), (0, 15), (0, 16), (0, 31), (0, 32), (1, 30), (1, 31), (1, 32)]


class Case:
    pass


def machine_case(O, made, q, pb, lanes=None, full=()):
    """made: [(mains, pres, progs, tabs, public values)], one per proof of ONE machine -> the machine, its oracle-made proofs, the catalogue over them: every site
    on the (proof, query) pairs in `full`, one site of each kind on the other lanes"""
    import recursion_machine as RM
    mains, pres, progs, tabs, _ = made[0]
    c = Case()
    c.q, c.pb = q, pb
    c.lns = [m.shape[0].bit_length() - 1 for m in mains]
    c.widths = [m.shape[1] for m in mains]
    c.pws = [0 if p is None else p.shape[1] for p in pres]
    c.progs, c.tabs = progs, tabs
    prm = O.default_params(1, q, pb)
    c.vk = [int(x) for x in O.machine_setup(pres, c.lns, prm)]
    c.chips = [dict(ln=c.lns[i], W=c.widths[i], Pw=c.pws[i], prog=progs[i], tab=tabs[i]) for i in range(len(mains))]
    c.proofs = [O.prove_machine_keyed(m[0], m[1], m[2], m[3], m[4], prm).tobytes() for m in made]
    c.pubs = [list(m[4]) for m in made]
    c.sh = RM.MShape(c.chips, c.vk, q, pb, len(c.pubs[0]), len(made))
    c.lay, c.entries = machine_catalogue(c.sh, lanes)
    c.entries = [f for f in c.entries if f.q is None or (f.p, f.q) in full] + thinned([f for f in c.entries if f.q is not None and (f.p, f.q) not in full])
    assert all(len(p) == 4 * c.lay.words for p in c.proofs)
    return c


def byte_case(O):
    import machines as M
    return machine_case(O, [M.byte_machine(7, 3, seed) for seed in (1, 2)], 3, 1, full=FIRST_AND_LAST)


def mixed_case(O):
    import machines as M
    return machine_case(O, [M.sp1_shaped_machine(SP1_SMALL, seed=5, shard=s, pre=((3, 8),)) for s in (0, 1)], 3, 1, full=FIRST_AND_LAST)


def wide_case(O):
    import machines as M
    return machine_case(O, [M.byte_machine(5, 3, seed) for seed in (1, 2)], WIDE_Q, 1, lanes=WIDE_LANES)


def shard_case(O, air, log_n=6):
    """two 2^log_n x 16 shard proofs of three queries: version 1, or version 7 under the synthetic AIR as a constraint program.  At 2^6 the two proofs make 48
    chains, whole workgroups of the chain kernel; at 2^5 they make 42: a partial last workgroup"""
    c = Case()
    c.log_n, c.width, c.q, c.pb, c.air = log_n, 16, 3, 1, air
    c.pubs = [[5, 6, 30 + s] for s in range(2)]
    c.prog = O.air_synthetic(c.width, 3) if air else None
    prm = O.default_params(1, c.q, c.pb)
    traces = [O.gen_trace(SEED, 40 + s, c.log_n, c.width) for s in range(2)]
    c.proofs = [(O.prove_shard_air(c.prog, traces[s], c.pubs[s], prm) if air else O.prove_shard(traces[s], c.pubs[s], prm)).tobytes() for s in range(2)]
    c.lay, c.entries = shard_catalogue(c.log_n, c.width, c.q, 2, air)
    assert all(len(p) == 4 * c.lay.words for p in c.proofs)
    return c
