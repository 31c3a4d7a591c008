"""The executable statement of fcmf_sample_token's contract (include/fcmf_hip.h) in float64 numpy on the STORED values, ties
handled by value, and the precondition under which a float32 kernel must reproduce it exactly.  Plain module: no fixtures, and
nothing here calls the library.

For a row x (stored values upcast to float64), temperature T, top_k, top_p, counter c and seed:
  K  every column when top_k == 0 or top_k >= V, else { j : x_j >= the top_k-th largest value } (ties at it all kept);
  z = x / T, p = softmax of z over K;
  M(x_j) = the mass of the columns of K with a value strictly above x_j;  N = { j in K : M(x_j) < top_p } (all of K at top_p == 1);
  id = argmax over N of z_j + g_j (the lower column on a tie), g = -log(-log(u)), u = ((h >> 9) + 0.5) 2^-23,
  h_j = _hash32(seed, ((c & (2^44 - 1)) << 20) | j) of rowwise_ref;  a -inf column is never drawn;
  logp = x_id - logsumexp(x): temperature 1, unfiltered.

DECIDED rows.  A float32 kernel cannot place a column whose M is within rounding of top_p, nor order two perturbed logits that
nearly tie.  With EPS = 1e-4 (the project's bound on a float32 log-softmax over the vocabulary, test_topk_gpu.py: a mass is a
sum of such terms) and LEAD = 1e-3 (about 30 times the float32 error of z + g at |z| <= 50):
  A, the ambiguous set = the columns of K with |M - top_p| <= EPS;  C, the certain set = those with M < top_p - EPS;
  the columns with M == 0, the row's maxima, are certain whatever top_p is: the contract keeps them unconditionally, and M == 0 is
  an empty sum, which no arithmetic rounds (without this a top_p below EPS would leave every row undecided);
  a row is decided when the argmax of z + g over C | A lies in C and leads the runner-up of C | A by at least LEAD.
Tests assert `decided` for every row they use, on the CPU, and choose their seeds so that it holds."""
import numpy as np

from rowwise_ref import _hash32

EPS, LEAD = 1e-4, 1e-3
CTR_MASK = (1 << 44) - 1


def hash_row(seed, ctr, V):
    """h_j for the columns 0 .. V-1 of a row with counter `ctr`: uint64 array holding 32-bit values"""
    pair = np.uint64((int(ctr) & CTR_MASK) << 20) | np.arange(V, dtype=np.uint64)
    return _hash32(seed, pair)


def uniform_row(seed, ctr, V):
    return ((hash_row(seed, ctr, V) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel_row(seed, ctr, V):
    return -np.log(-np.log(uniform_row(seed, ctr, V)))


def counter(sample, chain, t, num_chains, max_len):
    """the counter of (running sample index, chain, round) in decoding.sample_rounds"""
    return (sample * num_chains + chain) * max_len + t


def filtered(x, temperature=1.0, top_k=0, top_p=1.0):
    """x float64 [V] -> (K bool [V], z [V], M [V]: the mass strictly above each column's value among K, NaN outside K)"""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    if top_k == 0 or top_k >= V:
        K = np.ones(V, dtype=bool)
    else:
        K = x >= np.sort(x)[V - top_k]
    z = x / temperature
    zk = z[K]
    e = np.exp(zk - zk.max())
    p = e / e.sum()
    vals, inv = np.unique(x[K], return_inverse=True)            # ascending distinct stored values; ties share one entry
    mass = np.zeros(vals.shape[0])
    np.add.at(mass, inv, p)
    above = np.concatenate((np.cumsum(mass[::-1])[::-1][1:], [0.0]))      # mass of the distinct values strictly above
    M = np.full(V, np.nan)
    M[K] = above[inv]
    return K, z, M


def logp_of(x, j):
    x = np.asarray(x, dtype=np.float64)
    m = x.max()
    return x[j] - (m + np.log(np.exp(x - m).sum()))


def sample_row(x, ctr, seed, temperature=1.0, top_k=0, top_p=1.0):
    """-> (id, logp, decided, lead): the contract's draw, and whether the row is decided (module header)"""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    K, z, M = filtered(x, temperature, top_k, top_p)
    with np.errstate(invalid="ignore"):
        if top_p >= 1.0:
            N, C, A = K.copy(), K.copy(), np.zeros(V, dtype=bool)
        else:
            N = K & (M < top_p)
            C = K & ((M < top_p - EPS) | (M == 0.0))
            A = K & (np.abs(M - top_p) <= EPS) & ~C
    v = z + gumbel_row(seed, ctr, V)
    v[np.isneginf(x)] = -np.inf
    pick = lambda mask: int(np.argmax(np.where(mask, v, -np.inf)))      # (np.argmax: the first, i.e. lower, column on a tie)
    j = pick(N)
    assert N[j] and np.isfinite(v[j]), "no column to draw"
    both = C | A
    jb = pick(both)
    rest = both.copy()
    rest[jb] = False
    lead = float(v[jb] - np.where(rest, v, -np.inf).max()) if rest.any() else float("inf")
    ok = bool(C[jb]) and jb == j and lead >= LEAD
    return j, float(logp_of(x, j)), ok, lead


def sample_rows(X, ctrs, seed, temperature=1.0, top_k=0, top_p=1.0):
    """X [rows, V] (anything np.asarray takes, already float64) -> (ids int64 [rows], logp float64 [rows], decided bool [rows], leads)"""
    out = [sample_row(x, c, seed, temperature, top_k, top_p) for x, c in zip(np.asarray(X, dtype=np.float64), ctrs)]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out]))


def sample_chains(step_logits, sample, num_chains, start_id, sep_id, max_len, seed, temperature=1.0, top_k=0, top_p=1.0):
    """the sampling loop of ONE sample, stated per chain: chain c starts at [start_id]; round t draws sample_row(step_logits(seq),
    counter(sample, c, t)) and appends it; a chain ends at sep_id or after max_len draws; its score is the sum of the logp.
    step_logits(seq) -> the logits [V] after the sequence (a step on the last token reads seq[-1] only).
    -> ([(score, ids)] per chain, every draw decided?, the smallest lead)"""
    chains, all_ok, worst = [], True, float("inf")
    for c in range(num_chains):
        seq, score = [int(start_id)], 0.0
        for t in range(max_len):
            j, lp, ok, lead = sample_row(step_logits(seq), counter(sample, c, t, num_chains, max_len), seed, temperature, top_k, top_p)
            all_ok, worst = all_ok and ok, min(worst, lead)
            seq.append(j)
            score += lp
            if j == sep_id:
                break
        chains.append((score, seq))
    return chains, all_ok, worst
