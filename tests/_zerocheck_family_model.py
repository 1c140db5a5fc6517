"""Python model of the FAMILY of zerocheck-shaped proofs over FRI commitments: the prover's round loop, the verifier's replay, `sizes`,
`pow_transcript` and `flat` once, for the protocols of include/zkmle.h "Zerocheck of a product of committed tables", ".. of a Plonk gate ..",
"Wiring ..", "Plonk ..", "Lookup ..", "Plonk with lookups .." and ".. on column commitments".  tests/_zerocheck_model.py,
_zerocheck_gate_model.py, _wiring_model.py, _plonk_model.py, _lookup_model.py, _plonk_lookup_model.py and _plonk_lookup_columns_model.py bind
their public names to it and keep what is theirs alone (the instances, the helper tables, the summand and the round message written from the
definition, and the protocol's written definition); it imports none of them.  A protocol is a Proto:

  tag        tag(d), or tag(d, l) where `claimed` is set; the statement is the tag, the given roots, the l public values as 32-byte elements
  given      the number of given tables
  nodes      the round message is sent at X = 0 .. nodes - 1
  first      the number of challenges drawn straight behind the statement
  phases     ((roots, challenges), ..): per helper phase, how many roots are appended and how many challenges are drawn behind them; tau_0 ..
             tau_{d-1} are drawn behind the last.  This ONE list drives the prover (which makes and commits the phase's tables there) and the
             verifier (which reads the roots from the proof)
  helpers    helpers(i, tables so far, challenges so far, p, cheat) -> (phase i's tables, keys to add to the proof's dict)
  summand    summand(v, ids, ch): the summand at a point, v = the values of the opened tables and of E there, ids of the three id tables
  message    message(tables, explicit tables, ch, p) -> (g(0) .. g(nodes - 1) as sent, the nodes of the summand's own round polynomial or None)
  explicit   None, or explicit(d, pub) -> the explicit tables folded alongside: the three id tables, then PI where there are public inputs
  claimed    None (the claimed sum is 0), or claimed(pub, tau, ch, p) = alpha^3 sum_x PI[x] E[x]
  opening    the opening's model: _fri_ml_batch_model, _fri_ml_wide_model, or _fri_ml_columns_model with `widths`

  prover     statement; the phases; E = eq_table(tau); d rounds: the message, in round 0 of a cheating prover g(1) = claimed - g(0), the nodes
             absorbed, r_l drawn, every table folded by mle_fold_last; the opening of all commitments at z, z[d - 1 - l] = r_l
  verifier   statement; the phases; per round the nodes absorbed, each in [0, p), g(0) + g(1) = the running claim, r_l, the next claim by
             Lagrange's formula; the last claim against the summand on the opened values; the opening's verifier (and the proof-of-work).
             -> (ok, the number of the first failed check): 0 .. d - 1 a round (0 also a public value outside [0, p)), d the last claim,
             d + 1 the opening
Everything is Python integers; nothing here knows how the library works."""
import collections

import numpy as np

import _fri_ml_grouped_model as GM
import _fri_ml_model as ML
import _fri_pcs_model as PM
import _grind_model as GR
import _ntt_model as NM
from oracle import pymodel as M

be32 = ML.be32
WIRES = 3

Proto = collections.namedtuple("Proto", "tag given nodes first phases helpers summand message explicit claimed opening widths")
Proto.__new__.__defaults__ = (0, (), None, None, None, None, None, None, None)         # from `first` on


# ---- the pieces --------------------------------------------------------------------------------------------------------------------------
def interpolate(g, r, p):
    """the polynomial through (0, g[0]) .. (len(g) - 1, g[-1]) at r, by Lagrange's formula"""
    out = 0
    for i in range(len(g)):
        num, den = 1, 1
        for j in range(len(g)):
            if j != i:
                num, den = num * (r - j) % p, den * (i - j) % p
        out += g[i] * num * pow(den, -1, p)
    return out % p


def eq_at(z, tau, p):
    out = 1
    for a, b in zip(z, tau):
        out = out * ML.eq1(a, b, p) % p
    return out


def inv0(a, p):
    return 0 if a % p == 0 else pow(a, -1, p)


def id_tables(d):
    n = 1 << d
    return [[j * n + x for x in range(n)] for j in range(WIRES)]


def id_at(j, z, d, p):
    """the closed form of the multilinear extension of id_j at z: variable 0 is the most significant index bit"""
    return (j * (1 << d) + sum((1 << (d - 1 - i)) * zi for i, zi in enumerate(z))) % p


def commit_like(cm, table, hasher):
    """the model commitment of `table` with the shape of the model commitment `cm`"""
    mod = GM if cm.get("log_group", 0) else PM
    return mod.commit(cm["field"], table, cm["b"], cm["coset"], hasher)


def statement(proto, tr, roots, d, p, pub=()):
    """absorbs the statement -> the challenges drawn straight behind it"""
    tr.append(proto.tag(d, len(pub)) if proto.claimed else proto.tag(d))
    for r in roots:
        tr.append(r)
    for v in pub:
        tr.append(be32(v % p))
    return [tr.challenge(p) for _ in range(proto.first)]


def helpers(proto, tr, h_roots, d, p, drawn=()):
    """the helper phases and tau -> the phases' challenges, then tau as a list.  h_roots: the helper roots (a verifier's), or
    phase(i, the challenges so far) -> phase i's roots (the prover's, which makes and commits the tables there)"""
    out, at = [], 0
    for i, (nroots, ndraw) in enumerate(proto.phases):
        for r in h_roots(i, list(drawn) + out) if callable(h_roots) else h_roots[at:at + nroots]:
            tr.append(r)
        at += nroots
        out += [tr.challenge(p) for _ in range(ndraw)]
    return out + [[tr.challenge(p) for _ in range(d)]]


def pow_transcript(proto, d, f, bits, nonce=None, prefix=b""):
    """the transcript of a proof with the proof-of-work step: it stands in front of the first index, behind the samples of the statement and
    the phases, d (tau), d (the rounds), 1 (the opening's gamma) and R (its rounds)"""
    tr = GR.PowTranscript(bits, proto.first + sum(n for _, n in proto.phases) + 2 * d + 1 + (d - f), nonce)
    tr.append(prefix)
    return tr


def sizes(proto, d, b, f, Q, a=1, grouped=False):
    """(nround,) + (nhroots,) where there are helpers + the opening model's five counts"""
    nh = sum(n for n, _ in proto.phases)
    rest = proto.opening.sizes(list(proto.widths), d, b, f, Q) if proto.widths else proto.opening.sizes(proto.given + nh, d, b, f, Q, a, grouped)
    return (proto.nodes * d,) + ((nh,) if proto.phases else ()) + rest


# ---- the prover --------------------------------------------------------------------------------------------------------------------------
def prove_rounds(proto, cms, pub, f, Q, a=1, tr=None, hasher=M.keccak256, cheat=None, commit=None):
    """-> the proof as a dict; `cms`: the model commitments of the given tables, all alike; `commit(table)`: the model commitment of a helper
    table (commit_like on the first by default; the columns' helpers go into one commitment per phase); `tr` is advanced.  The statement
    is not checked."""
    c0 = cms[0]
    field, d = c0["field"], c0["d"]
    p = NM.MODULUS[field]
    tr = M.Transcript() if tr is None else tr
    roots = [c["root"] for c in cms]
    tabs = [list(t) for c in cms for t in (c["coeffs"] if proto.widths else [c["coeffs"]])]
    assert len(tabs) == proto.given and len(pub) <= 1 << d
    commit = (lambda t: commit_like(c0, t, hasher)) if commit is None else commit
    hcms, extras = [], {}

    def phase(i, drawn):
        new, more = proto.helpers(i, tabs, drawn, p, cheat)
        made = [proto.opening.commit(field, new, c0["b"], c0["coset"], hasher)] if proto.widths else [commit(t) for t in new]
        tabs.extend(new)
        hcms.extend(made)
        extras.update(more)
        return [c["root"] for c in made]

    ch = statement(proto, tr, roots, d, p, pub)
    *more, tau = helpers(proto, tr, phase, d, p, ch)
    ch = ch + more
    K = len(tabs)
    tabs.append(ML.eq_table(tau, p))
    extra = proto.explicit(d, pub) if proto.explicit else []
    claimed = proto.claimed(pub, tau, ch, p) if proto.claimed else 0
    polys, rs, own_first = [], [], 0
    for l in range(d):
        g, own = proto.message(tabs, extra, ch, p)
        if l == 0 and own is not None:
            own_first = (own[0] + own[1]) % p
        if cheat and l == 0:
            g[1] = (claimed - g[0]) % p
        polys.append(g)
        for e in g:
            tr.append(be32(e))
        r = tr.challenge(p)
        rs.append(r)
        tabs, extra = [ML.mle_fold_last(field, t, r) for t in tabs], [ML.mle_fold_last(field, t, r) for t in extra]
    z = rs[::-1]
    every = list(cms) + hcms
    op = proto.opening.open_columns(every, [z], f, Q, tr, hasher) if proto.widths else proto.opening.open_batch(every, [z], f, Q, a, tr, hasher)
    assert [row[0] for row in op["ys"]] == [t[0] for t in tabs[:K]] and tabs[K][0] == eq_at(z, tau, p)
    assert [t[0] for t in extra[:WIRES]] == [id_at(j, z, d, p) for j in range(WIRES)][:len(extra)]
    assert not proto.widths or op["widths"] == list(proto.widths)
    out = {"field": field, "d": d, "roots": roots, "polys": polys, "challenges": rs, "opening": op, "nonce": getattr(tr, "nonce", None) or 0}
    if proto.claimed:
        out.update(pub=list(pub), own_first_sum=own_first)
    if proto.phases:
        out.update(h_roots=[c["root"] for c in hcms], drawn=ch + tau)
    else:
        out["tau"] = tau
    out.update(extras)
    return out


# ---- the verifier ------------------------------------------------------------------------------------------------------------------------
def replay(proto, pr, roots=None, pub=None, tr=None, hasher=M.keccak256):
    """`roots`, `pub`: the verifier's own roots and public values, the proof's unless given -> (ok, the number of the first check that failed
    or None)"""
    field, d, op = pr["field"], pr["d"], pr["opening"]
    p = NM.MODULUS[field]
    tr = M.Transcript() if tr is None else tr
    roots = pr["roots"] if roots is None else roots
    pub = pr.get("pub", ()) if pub is None else pub
    h_roots = pr.get("h_roots", [])
    ch = statement(proto, tr, roots, d, p, pub)
    *more, tau = helpers(proto, tr, h_roots, d, p, ch)
    ch = ch + more
    fits = len(pub) <= 1 << d
    failed = None if fits and all(0 <= v < p for v in pub) else 0
    cur, rs = proto.claimed(pub, tau, ch, p) if proto.claimed and fits else 0, []
    for l in range(d):
        g = pr["polys"][l]
        for e in g:
            tr.append(be32(e % p))
        if failed is None and (any(not 0 <= e < p for e in g) or (g[0] + g[1]) % p != cur):
            failed = l
        rs.append(tr.challenge(p))
        cur = interpolate(g, rs[l], p)
    z = rs[::-1]
    ys = [row[0] for row in op["ys"]]
    want = proto.summand(ys + [eq_at(z, tau, p)], [id_at(j, z, d, p) for j in range(WIRES)], ch) % p
    if failed is None and cur != want:
        failed = d
    own = dict(op, own_roots=list(roots) + list(h_roots), points=[z], **({"widths": list(proto.widths)} if proto.widths else {}))
    good = proto.opening.verify(own, tr, hasher) and getattr(tr, "pow_ok", None) is not False
    if failed is None and not good:
        failed = d + 1
    return failed is None, failed


# ---- the C ABI's layout ------------------------------------------------------------------------------------------------------------------
def mont(zk, field, ints):
    canon = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), np.uint64).reshape(-1, 4).copy()
    out = np.zeros_like(canon)
    if canon.shape[0]:
        assert zk.lib().zk_vec_from_canonical(field, canon.ctypes.data_as(zk._lib.u64p), canon.shape[0], out.ctypes.data_as(zk._lib.u64p)) == 0
    return out


def flat(proto, zk, pr):
    """the proof as the C outputs: polys (d, nodes, 4), challenges (d, 4), own_roots (the given ones, 32), and the opening's arrays of its
    model's flat under their names there with ys as (K, 4) and the opening's round polynomials as open_polys / open_challenges; with helpers
    h_roots (.., 32) and drawn (.. + d, 4), without them tau (d, 4); with public inputs pub (l, 4)"""
    field, d = pr["field"], pr["d"]
    fl = proto.opening.flat(zk, pr["opening"])
    fl["open_polys"], fl["open_challenges"] = fl.pop("polys"), fl.pop("challenges")
    fl["ys"] = fl["ys"].reshape(-1, 4)
    fl["own_roots"] = np.frombuffer(b"".join(pr["roots"]), np.uint8).reshape(-1, 32).copy()
    fl.update(polys=mont(zk, field, [e for g in pr["polys"] for e in g]).reshape(d, proto.nodes, 4), challenges=mont(zk, field, pr["challenges"]))
    if proto.phases:
        fl.update(h_roots=np.frombuffer(b"".join(pr["h_roots"]), np.uint8).reshape(-1, 32).copy(), drawn=mont(zk, field, pr["drawn"]))
    else:
        fl["tau"] = mont(zk, field, pr["tau"])
    if proto.claimed:
        fl["pub"] = mont(zk, field, pr["pub"])
    return fl
