"""RandomTape (reference src/random.rs:15-31) and the draw order of every prover, literally, on transcript_model.Transcript — the checker of
csrc/random_tape_host.hpp and of sbn_random_tape_* / sbn_*_draw_rnd.

Each draw_* returns the list of integers the matching prove call takes as rnd (include/sbn254.h), produced by the reference's calls in the reference's
order, cited by line.  Scalars are Python integers."""
from transcript_model import Transcript
import polyeval_model as pm
import r1cs_proof_model as rpm
import sparse_eval_model as sem

SNARK_NAME = b"snark_proof"                     # snark.rs:438
NIZK_NAME = b"proof"                            # snark.rs:210


class RandomTape:
    def __init__(self, name, init):
        """RandomTape::new (random.rs:15-23) with the scalar OsRng gives there handed in"""
        self.tape = Transcript(name)
        self.tape.append_scalar(b"init_randomness", init)

    def random_scalar(self, label):             # :25-27
        return self.tape.challenge_scalar(label)

    def random_vector(self, label, n):          # :29-31
        return [self.tape.challenge_scalar(label) for _ in range(n)]


def log2(n):
    assert n >= 1 and n & (n - 1) == 0
    return n.bit_length() - 1


def draw_zk_sumcheck(t, num_rounds, n):
    """ZKSumcheckInstanceProof::prove_cubic_with_additive_term (n = 4) / prove_quad (n = 3)"""
    out = t.random_vector(b"blinds_poly", num_rounds)                  # sumcheck.rs:483, :673
    out += t.random_vector(b"blinds_evals", num_rounds)                # :484, :674
    for _ in range(num_rounds):                                        # DotProductProof::prove, once a round (:600, :770)
        out += t.random_vector(b"d_vec", n)                            # nizk/mod.rs:326
        out.append(t.random_scalar(b"r_delta"))                        # :327
        out.append(t.random_scalar(b"r_beta"))                         # :328
    return out


def draw_polyeval(t, lg, beta_label=b"r_delta"):
    """DotProductProofLog::prove (nizk/mod.rs:458-468).  beta_label: the reference draws r_beta under b"r_delta" (:460); the parameter exists so that a
    test can show that the label matters"""
    d = t.random_scalar(b"d")                                          # :458
    r_delta = t.random_scalar(b"r_delta")                              # :459
    r_beta = t.random_scalar(beta_label)                               # :460
    v1 = t.random_vector(b"blinds_vec_1", lg)                          # :463
    v2 = t.random_vector(b"blinds_vec_2", lg)                          # :464
    out = [d, r_delta, r_beta]
    for i in range(lg):                                                # :465-467: (v1[i], v2[i])
        out += [v1[i], v2[i]]
    return out


def draw_r1cs_proof(t, num_cons, num_vars, beta_label=b"r_delta"):
    """R1CSProof::prove (r1csproof.rs:241-459) at a padded shape"""
    nx, ell = log2(num_cons), log2(num_vars)
    ny = ell + 1
    left, right = pm.factored_lens(ell)
    out = t.random_vector(b"poly_blinds", 1 << left)                   # r1csproof.rs:225
    out += draw_zk_sumcheck(t, nx, 4)                                  # :295
    out += [t.random_scalar(l) for l in (b"Az_blind", b"Bz_blind", b"Cz_blind", b"prod_Az_Bz_blind")]      # :318-321
    out += [t.random_scalar(b"t1"), t.random_scalar(b"t2")]            # KnowledgeProof::prove, nizk/mod.rs:44-45
    out += [t.random_scalar(l) for l in (b"b1", b"b2", b"b3", b"b4", b"b5")]      # ProductProof::prove, :181-185
    out.append(t.random_scalar(b"r"))                                  # EqualityProof::prove, :108
    out += draw_zk_sumcheck(t, ny, 3)                                  # r1csproof.rs:394
    out.append(t.random_scalar(b"blind_eval"))                         # :410
    out += draw_polyeval(t, right, beta_label)                         # PolyEvalProof::prove, :413
    out.append(t.random_scalar(b"r"))                                  # the second EqualityProof
    assert len(out) == rpm.sizes(num_cons, num_vars)[0]
    return out


def draw_sparse_eval(t, nx, ny, num_ops, batch, kzg=False, beta_label=b"r_delta"):
    """HashLayerProof::prove's three openings in the order it makes them: derefs (the Hyrax build only), ops, mem"""
    s = sem.Shape(nx, ny, num_ops, batch)
    out = []
    for k in ("ops", "mem") if kzg else ("derefs", "ops", "mem"):
        out += draw_polyeval(t, s.lg[k], beta_label)
    return out


def draw_snark(t, comm, kzg=False, beta_label=b"r_delta"):
    """SNARK::prove: ONE tape (snark.rs:438) through R1CSProof::prove and then R1CSEvalProof::prove; comm: snark_model's commitment dict"""
    out = draw_r1cs_proof(t, comm["nc"], comm["nv"], beta_label)
    return out + draw_sparse_eval(t, log2(comm["nc"]), log2(2 * comm["nv"]), comm["N"], comm["batch"], kzg, beta_label)


def draw_nizk(t, inst, beta_label=b"r_delta"):
    """NIZK::prove: R1CSProof::prove's draws (snark.rs:210); inst: a snark_model / nizk_model instance with nc, nv"""
    return draw_r1cs_proof(t, inst.nc, inst.nv, beta_label)


def to_bytes(scalars):
    return b"".join(int(x).to_bytes(32, "little") for x in scalars)
