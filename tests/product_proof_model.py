"""The layered product-circuit argument (ProductCircuitEvalProofBatched, product_tree.rs:251-392 prove, :394-... verify) in plain Python
integers: a prover AND a verifier, the checker of sbn_product_proof_prove.

Written from the protocol — the batched cubic sumcheck (sumcheck.rs:165-330, its verifier :35-85), the round polynomial
(unipoly.rs) and the layer loop — on top of transcript_model.py (Merlin) and pyref.py (eq, bind, round sums).  It shares no code
with the library.  Scalars are ints mod R; a proof is the four flat outputs of the library call as lists of ints:
  polys   per layer (top first), per round: [c0, c1, c2, c3]
  claims  per layer: (claims_prod_left[n_circ], claims_prod_right[n_circ]);  claims_dotp = (left, right, weight)
  rand    the final point (r_layer of the last layer first), claims_final: claims_to_verify behind the last layer
"""
import pyref
import transcript_model as tm

R = pyref.R


def product_circuit(inp):
    """ProductCircuit::new (product_tree.rs:22-57): layer j = (left, right) halves of the products so far; the input is layer 0"""
    layers, cur = [], list(inp)
    while len(cur) >= 2:
        h = len(cur) // 2
        layers.append((cur[:h], cur[h:]))
        cur = [cur[i] * cur[h + i] % R for i in range(h)]
    return layers


def circuit_evaluate(layers):
    l, r = layers[-1]
    assert len(l) == 1 and len(r) == 1
    return l[0] * r[0] % R


def dotp_evaluate(d):
    left, right, weight = d
    return sum(a * b * c for a, b, c in zip(left, right, weight)) % R


def _sumcheck_prove(tr, claim, rounds, inst, coeffs):
    """prove_cubic_batched: inst = [[A, B, C], ...] (lists, bound in place per round; a shared C is the same list object in several
    instances and is bound once) -> (polys, challenges, [(A[0], B[0], C[0])])"""
    e, polys, rs = claim, [], []
    for _ in range(rounds):
        e0 = e2 = e3 = 0
        for (A, B, C), c in zip(inst, coeffs):
            s0, s2, s3 = pyref.sc_eval_cubic(A, B, C)
            e0 += c * s0; e2 += c * s2; e3 += c * s3
        co, r, e = tm.sumcheck_round_step(tr, e, e0 % R, e2 % R, e3 % R)
        polys.append(co); rs.append(r)
        done = {}
        for t in inst:
            for k in range(3):
                if id(t[k]) not in done:
                    done[id(t[k])] = (t[k], pyref.bind_top(t[k], r))      # (the old list is kept alive: its id stays unique)
                t[k] = done[id(t[k])][1]
    return polys, rs, [(A[0], B[0], C[0]) for A, B, C in inst]


def prove(tr, circuits, dotps, skip_zero_round_layer=False):
    """circuits: [product_circuit(...)] of equal depth; dotps: [(left, right, weight)] of half the input length.  `tr` moves on.
    skip_zero_round_layer: leave the top layer's transcript work out (what a prover that starts at the first real sumcheck does) —
    a wrong proof, for the verifier's test."""
    n, L = len(circuits), len(circuits[0])
    claims_to_verify = [circuit_evaluate(c) for c in circuits]
    rand, polys, claims, claims_dotp = [], [], [], ([], [], [])
    for layer in range(L - 1, -1, -1):
        half = len(circuits[0][layer][0])
        rounds = half.bit_length() - 1
        assert len(rand) == rounds
        eq = pyref.eq_evals(rand)
        inst = [[list(c[layer][0]), list(c[layer][1]), eq] for c in circuits]
        with_dotp = layer == 0 and len(dotps) > 0
        if with_dotp:
            claims_to_verify = claims_to_verify + [dotp_evaluate(d) for d in dotps]
            inst += [[list(d[0]), list(d[1]), list(d[2])] for d in dotps]
        if rounds == 0 and skip_zero_round_layer:
            lefts, rights = [c[layer][0][0] for c in circuits], [c[layer][1][0] for c in circuits]
            polys.append([]); claims.append((lefts, rights))
            claims_to_verify = list(lefts)        # no r_layer was drawn: nothing to fold with
            rand = [0]
            continue
        coeffs = [tr.challenge_scalar(b"rand_coeffs_next_layer") for _ in claims_to_verify]
        claim = sum(a * b for a, b in zip(claims_to_verify, coeffs)) % R
        lp, rs, fin = _sumcheck_prove(tr, claim, rounds, inst, coeffs)
        lefts, rights = [f[0] for f in fin[:n]], [f[1] for f in fin[:n]]
        for a, b in zip(lefts, rights):
            tr.append_scalar(b"claim_prod_left", a); tr.append_scalar(b"claim_prod_right", b)
        if with_dotp:
            claims_dotp = ([f[0] for f in fin[n:]], [f[1] for f in fin[n:]], [f[2] for f in fin[n:]])
            for a, b, c in zip(*claims_dotp):
                tr.append_scalar(b"claim_dotp_left", a); tr.append_scalar(b"claim_dotp_right", b); tr.append_scalar(b"claim_dotp_weight", c)
        r_layer = tr.challenge_scalar(b"challenge_r_layer")
        claims_to_verify = [(a + r_layer * (b - a)) % R for a, b in zip(lefts, rights)]
        rand = [r_layer] + rs
        polys.append(lp); claims.append((lefts, rights))
    return {"polys": polys, "claims": claims, "claims_dotp": claims_dotp, "rand": rand, "claims_final": claims_to_verify}


def verify(tr, proof, claims_prod, claims_dotp_in, n_layers):
    """the verifier's layer loop: claims_prod = ProductCircuit::evaluate of every circuit, claims_dotp_in = DotProductCircuit::evaluate of every
    dot-product circuit.  Returns (ok, claims_to_verify, rand): what is left to check is layer 0 of circuit i at rand (and the dot-product claims)."""
    n = len(claims_prod)
    claims_to_verify, rand = list(claims_prod), []
    if len(proof["polys"]) != n_layers or len(proof["claims"]) != n_layers:
        return False, None, None
    for i in range(n_layers):
        last = i == n_layers - 1
        if last:
            claims_to_verify = claims_to_verify + list(claims_dotp_in)
        coeffs = [tr.challenge_scalar(b"rand_coeffs_next_layer") for _ in claims_to_verify]
        e = sum(a * b for a, b in zip(claims_to_verify, coeffs)) % R
        if len(proof["polys"][i]) != i:
            return False, None, None
        rs = []
        for co in proof["polys"][i]:
            if len(co) != 4 or (2 * co[0] + co[1] + co[2] + co[3] - e) % R:      # degree 3; p(0) + p(1) = e
                return False, None, None
            tr.append_message(b"poly", b"UniPoly_begin")
            for c in co:
                tr.append_scalar(b"coeff", c)
            tr.append_message(b"poly", b"UniPoly_end")
            r = tr.challenge_scalar(b"challenge_nextround")
            rs.append(r)
            e = tm.unipoly_eval(co, r)
        lefts, rights = proof["claims"][i]
        if len(lefts) != n or len(rights) != n:
            return False, None, None
        for a, b in zip(lefts, rights):
            tr.append_scalar(b"claim_prod_left", a); tr.append_scalar(b"claim_prod_right", b)
        eq = 1
        for x, y in zip(rand, rs):
            eq = eq * (x * y + (1 - x) * (1 - y)) % R
        expected = sum(c * a * b * eq for c, a, b in zip(coeffs, lefts, rights)) % R
        if last:
            dl, dr, dw = proof["claims_dotp"]
            if not (len(dl) == len(dr) == len(dw) == len(claims_dotp_in)):
                return False, None, None
            for k in range(len(dl)):
                tr.append_scalar(b"claim_dotp_left", dl[k]); tr.append_scalar(b"claim_dotp_right", dr[k]); tr.append_scalar(b"claim_dotp_weight", dw[k])
                expected = (expected + coeffs[n + k] * dl[k] * dr[k] * dw[k]) % R
        if expected != e:
            return False, None, None
        r_layer = tr.challenge_scalar(b"challenge_r_layer")
        claims_to_verify = [(a + r_layer * (b - a)) % R for a, b in zip(lefts, rights)]
        rand = [r_layer] + rs
    ok = rand == list(proof["rand"]) and claims_to_verify == list(proof["claims_final"])
    return ok, claims_to_verify, rand


def evaluate_mle(Z, r):
    """DensePolynomial::evaluate (hyrax.rs:217-222)"""
    return sum(a * b for a, b in zip(Z, pyref.eq_evals(r))) % R


# ---- the library call's flat byte outputs <-> the proof dictionary -------------------------------------------------------------

def _ints(b):
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(b) // 32)]


def proof_from_flat(out_polys, out_claims, out_rand, out_claims_final, n_circ, n_dotp, n_layers):
    p, c = _ints(out_polys), _ints(out_claims)
    polys, claims, o = [], [], 0
    for k in range(n_layers):
        polys.append([p[4 * (o + j):4 * (o + j) + 4] for j in range(k)]); o += k
        claims.append((c[2 * n_circ * k:2 * n_circ * k + n_circ], c[2 * n_circ * k + n_circ:2 * n_circ * (k + 1)]))
    d = c[2 * n_circ * n_layers:]
    return {"polys": polys, "claims": claims, "claims_dotp": (d[:n_dotp], d[n_dotp:2 * n_dotp], d[2 * n_dotp:3 * n_dotp]),
            "rand": _ints(out_rand), "claims_final": _ints(out_claims_final)}


def proof_to_flat(proof):
    b = lambda xs: b"".join(int(x).to_bytes(32, "little") for x in xs)
    polys = b"".join(b(co) for lp in proof["polys"] for co in lp)
    claims = b"".join(b(l) + b(r) for l, r in proof["claims"]) + b"".join(b(x) for x in proof["claims_dotp"])
    return polys, claims, b(proof["rand"]), b(proof["claims_final"])
