"""The CIDEr-D scorer kernels (csrc/cider_kernel.hip: cook_refs, img_ngram, cider_img, the per-reference scan
`cider`, finish_fitness) on CHOSEN token rows, through nicnes_test_score_rows (Engine.test_score_rows): the
dispatch nicnes_evaluate* ends with, fed hypotheses a decode of a random theta never emits. Every comparison
is against oracle/cider_ref.py (pinned by tests/test_cider_oracle.py): per-row scores and greedy fitness to
1e-9 relative, the log-prob criteria to 1e-6 relative (the bounds of tests/test_gpu_parity.py)."""
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import cider_ref as CR      # noqa: E402

T = 16
VOCAB = 16383                # V1 = 16384: ids use all 14 bits of a key field
N_RAW = 40                   # ref_len_raw of the hand-built df tables
TOL, TOL_CRIT = 1e-9, 1e-6


# ---------------------------------------------------------------- helpers --------------------------
def row(*toks, T=T):
    r = np.zeros(T, np.int32)
    r[:len(toks)] = toks
    return r


def strs(rows):
    return [CR.array_to_str(r) for r in rows]


def oracle_scores(scorer, seq, gts, rpi=1):
    """CiderDOracle.score_one of every row of seq [rows, T] against the references of image row // rpi."""
    refs = [strs(g) for g in gts]
    return np.array([scorer.score_one(CR.array_to_str(seq[i]), refs[i // rpi]) for i in range(seq.shape[0])])


def close(got, ref, tol=TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) <= tol * np.maximum(1.0, np.abs(ref))


def assert_rows(got, ref, names=None, tol=TOL):
    ok = close(got, ref, tol)
    bad = np.argwhere(~ok)
    assert ok.all(), [(tuple(i), names[i[-1]] if names else None, float(got[tuple(i)]), float(ref[tuple(i)]))
                      for i in bad[:8]]


def load(eng, df, n_raw, gts, keys_vals=None):
    import nicnes
    keys, vals = keys_vals if keys_vals is not None else nicnes.df_table_arrays(df)
    eng.set_df_table(keys, vals, np.log(float(n_raw)))
    eng.set_batch(np.zeros((len(gts), eng.cfg.fc_feat_size), np.float32), gts)


def make_engine(vocab=VOCAB, seq_length=T, max_batch=128, max_members=2):
    import nicnes
    import nicnes.synthetic as S
    return nicnes.Engine(vocab_size=vocab, seq_length=seq_length, max_batch=max_batch, max_members=max_members,
                         noise_len=S.Dims(vocab).D, noise_seed=0)


@pytest.fixture(scope='module')
def eng():
    e = make_engine(max_members=512)
    yield e
    e.close()


# ---------------------------------------------------------------- case 1: hand-built rows ----------
A, Bk, C = 1, 8192, 16383          # lowest id, the top bit alone, every bit
DISTINCT16 = list(range(101, 117))
PAD_TOTAL = 100000
PAD_CAP = 1 << 18                  # nicnes_df_hash_capacity(100000): the power of two >= 2 n
WRAP_PRESENT, WRAP_ABSENT = (1008, 6742), (1006, 10503)     # df_hash & (PAD_CAP - 1) = PAD_CAP - 1, PAD_CAP - 3
WRAP_LATE = (16322, 3396, 11194, 7603)                      # ... = PAD_CAP - 1; among the last keys of the sorted table


def hand_cases():
    """[(name, hypothesis row, reference rows, closed-form score or None)]: one image per hypothesis."""
    rep4 = [4] * 16
    abab = [50, 60] * 8
    l16 = row(7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22)
    short_refs = [row(0), row(7, 0), l16]
    cases = [
        ('identical', row(5, 6, 7, 8, 9, 0), [row(5, 6, 7, 8, 9, 0)], 10.0),
        ('disjoint', row(*range(201, 217)), [row(*range(301, 317))], 0.0),
        # the string '0' against '0': the one unigram matches, orders 2-4 are empty: 1 / 4 * 10
        ('only_zero', row(0, 3, 4, 5), [row(0)], 2.5),
        ('no_zero_identical', row(*DISTINCT16), [row(*DISTINCT16)], 10.0),
        ('L2_vs_L1_2_16', row(7, 0), short_refs, None),
        ('L3_vs_L1_2_16', row(7, 8, 0), short_refs, None),
        ('L4_vs_L1_2_16', row(7, 8, 9, 0), short_refs, None),
        ('rep16_vs_tf1', row(*rep4), [row(4, 5, 6, 0)], None),
        ('rep16_vs_tf2', row(*rep4), [row(4, 4, 5, 0)], None),
        ('rep16_vs_tf3', row(*rep4), [row(4, 4, 4, 0)], None),
        ('rep16_vs_tf123', row(*rep4), [row(4, 5, 6, 0), row(4, 4, 5, 0), row(4, 4, 4, 0)], None),
        ('abab', row(*abab), [row(50, 60, 50, 60, 0), row(60, 50, 60, 50, 60, 50, 0)], None),
        ('abab_short', row(50, 60, 50, 60, 0), [row(*abab), row(60, 50, 0)], None),
        # 4-grams that differ from the hypothesis' in exactly one field (4th, 1st, 2nd, 3rd), and a swap
        ('top_ids_one_field', row(A, Bk, C, A, 0),
         [row(A, Bk, C, Bk, 0), row(C, Bk, C, A, 0), row(A, C, C, A, 0), row(A, Bk, Bk, A, 0), row(Bk, A, C, A, 0)], None),
        ('swap_ab_ba', row(A, C, 0), [row(C, A, 0)], None),
        ('swap_ab_ab', row(A, C, 0), [row(A, C, 0), row(C, A, 0)], None),
        # 8191 and 16383 differ in the top bit of a field only; 8192 and 0 likewise
        ('top_bit_8191', row(C, C, C, C, 0), [row(C, C, C, 8191, 0), row(8191, C, C, C, 0), row(C, C, C, C, 0)], None),
        ('top_bit_8192_vs_0', row(Bk, 5, 0), [row(0), row(Bk, 0), row(5, 0)], None),
        ('all_top', row(*([C] * 16)), [row(*([C] * 16)), row(*([C] * 15 + [8191])), row(*([Bk] * 16))], None),
        # every unigram at df = N (case 2): the hypothesis' unigram norm is exactly 0
        ('zero_weight_unigrams', row(*([21, 22, 23] * 5 + [21])), [row(21, 22, 23, 0), row(23, 22, 21, 21, 0)], None),
        # df = 4 N on both sides (case 2): negative weights through min()
        ('negative_weights', row(31, 32, 33, 0), [row(31, 31, 32, 33, 0), row(33, 32, 31, 0)], None),
        # bigrams whose df probe starts in the last slots of the padded table (case 2): one in the table, one not
        ('wrap_present', row(*WRAP_PRESENT, 0), [row(*WRAP_PRESENT, 5, 0)], None),
        ('wrap_absent', row(*WRAP_ABSENT, 0), [row(*WRAP_ABSENT, 0), row(*WRAP_ABSENT[::-1], 0)], None),
        ('wrap_late', row(*WRAP_LATE, 0), [row(9, *WRAP_LATE, 0)], None),
    ]
    return cases


NINE_REFS = [row(*[(3 * j + k) % 11 + 40 for k in range(3 + j)], 0) for j in range(9)]
NINE_HYP = row(40, 41, 42, 43, 44, 0)


def hand_batch(T_=T, scan=False):
    """seq [2, B, T_] (candidate 1 scores the next image's hypothesis: cross pairs), gts, names, closed forms."""
    cases = hand_cases()
    names = [c[0] for c in cases]
    hyps = [c[1][:T_] for c in cases]
    gts = [np.stack([r[:T_] for r in c[2]]) for c in cases]
    closed = [c[3] for c in cases]
    if scan:                # one image with 9 references sends the whole batch to the per-reference scan
        names.append('nine_refs')
        hyps.append(NINE_HYP[:T_])
        gts.append(np.stack([r[:T_] for r in NINE_REFS]))
        closed.append(None)
    h = np.stack(hyps)
    n_common = len(cases)
    seq = np.stack([h, np.concatenate([np.roll(h[:n_common], -1, 0), h[n_common:]])])
    return seq, gts, names, closed


def all_ngrams(rows_iter):
    out = set()
    for r in rows_iter:
        out.update(CR.precook(CR.array_to_str(r)).keys())
    return out


def edge_df(T_=T):
    """Every n-gram of the hand-built rows gets, in sorted order, one of: absent, 0.5, 1, 2, N, 4 N; then the
    two rows built for it: unigrams 21-23 at N (weight 0), 31-33 and their bigrams at 4 N (negative)."""
    seq, gts, _, _ = hand_batch(T_, scan=True)
    grams = sorted(all_ngrams(list(seq.reshape(-1, T_)) + [r for g in gts for r in g]),
                   key=lambda g: (len(g), tuple(int(w) for w in g)))
    cycle = [None, 0.5, 1.0, 2.0, float(N_RAW), 4.0 * N_RAW]
    df = {}
    for i, g in enumerate(grams):
        v = cycle[i % len(cycle)]
        if v is not None:
            df[g] = v
    for g in grams:
        ids = set(int(w) for w in g)
        if len(g) == 1 and ids <= {21, 22, 23}:
            df[g] = float(N_RAW)
        if len(g) <= 2 and ids <= {31, 32, 33}:
            df[g] = 4.0 * N_RAW
    df[tuple(str(t) for t in WRAP_PRESENT)] = 2.0
    df[tuple(str(t) for t in WRAP_LATE)] = 2.0
    df.pop(tuple(str(t) for t in WRAP_ABSENT), None)
    return {tuple(int(w) for w in g): v for g, v in df.items()}, grams


def np_df_hash(k):
    """df_hash of cider_kernel.hip on a uint64 array."""
    k = k.astype(np.uint64).copy()
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
    return k


def np_keys(n, toks):
    """packed keys of n-grams toks [m, n]"""
    key = np.full(toks.shape[0], n << 56, np.uint64)
    for k in range(n):
        key |= toks[:, k].astype(np.uint64) << np.uint64(42 - 14 * k)
    return key


def padded_df(df, grams):
    """df plus random n-grams (none of them an n-gram of the rows) up to PAD_TOTAL entries, first among them every
    candidate that hashes into the last 48 slots of the table: more than 48, so the probe chains there run off the
    end of the table and wrap. -> (table, how many such)"""
    used = set(tuple(int(w) for w in g) for g in grams)
    rng = np.random.Generator(np.random.PCG64(77))
    extra, tail = {}, 0
    for n, want in ((1, 4000), (2, 32000), (3, 32000), (4, PAD_TOTAL - 68000 - len(df))):
        toks = rng.integers(0, VOCAB + 1, (300000, n)) if n > 1 else rng.permutation(VOCAB + 1)[:, None]
        with np.errstate(over='ignore'):
            slot = np_df_hash(np_keys(n, toks)) & np.uint64(PAD_CAP - 1)
        at_end = slot >= np.uint64(PAD_CAP - 48)
        taken = 0
        for i in np.concatenate([np.flatnonzero(at_end), np.flatnonzero(~at_end)]):
            if taken >= want:
                break
            g = tuple(int(t) for t in toks[i])
            if g in used or g in extra:
                continue
            extra[g] = float(rng.integers(1, 4 * N_RAW))
            taken += 1
            tail += bool(at_end[i])
    out = dict(df)
    out.update(extra)
    return out, tail


# ---------------------------------------------------------------- case 3: mixed reference counts ----
def variant(rng, base, p_sub=0.2):
    L = int(rng.integers(1, T + 1))
    toks = [int(base[k % len(base)]) for k in range(L)]
    for k in range(L):
        if rng.random() < p_sub:
            toks[k] = int(rng.integers(1, VOCAB + 1))
    if L < T:
        toks[L - 1] = 0
    return row(*toks)


def gen_image(rng, k, n_hyp=2):
    base = rng.integers(1, VOCAB + 1, int(rng.integers(2, T + 1)))
    refs = np.stack([variant(rng, base) for _ in range(k)])
    hyps = np.stack([variant(rng, base) for _ in range(n_hyp)])
    return refs, hyps


def dense_image(rng, n_hyp=2):
    """8 references of 16 pairwise distinct tokens: 8 x 58 = 464 rows of the 512-row image table"""
    ids = rng.permutation(np.arange(1, VOCAB + 1))[:128].reshape(8, 16).astype(np.int32)
    hyps = ids[rng.integers(0, 8, n_hyp)].copy()
    hyps[:, 5] = ids[0, 0]
    return ids, hyps


def mixed_batch():
    """(seq [2, 67, T], gts of the image-path batch (65 images, k in 1..8, the dense one last), gts of the scan-path
    batch = the same 65 images + one of 9 and one of 20 references, df, n)."""
    rng = np.random.Generator(np.random.PCG64(5))
    ks = [1, 8] + [int(k) for k in rng.integers(1, 9, 62)]
    imgs = [gen_image(rng, k) for k in ks] + [dense_image(rng)] + [gen_image(rng, 9), gen_image(rng, 20)]
    gts = [i[0] for i in imgs]
    seq = np.stack([np.stack([i[1][c] for i in imgs]) for c in range(2)])
    df, n = CR.document_frequency_from_refs([strs(g) for g in gts])
    df = {tuple(int(w) for w in g): v for g, v in df.items()}
    return seq, gts[:65], gts, df, n


def order_hits(scorer, seq, gts):
    """[rows, 4] bool: the row has a non-zero sim term of order n against at least one of its references"""
    hits = np.zeros((seq.shape[0], 4), bool)
    for i in range(seq.shape[0]):
        vec, norm, length = scorer.counts2vec(CR.precook(CR.array_to_str(seq[i])))
        for r in strs(gts[i]):
            vr, nr, lr = scorer.counts2vec(CR.precook(r))
            hits[i] |= scorer.sim(vec, vr, norm, nr, length, lr) != 0
    return hits


# ---------------------------------------------------------------- shared runs -----------------------
def run_both_paths(eng, df, n_raw, seq, gts_img, gts_scan, keys_vals=None):
    """scores of seq's first len(gts_img) rows on the image-table path and of all rows on the scan path"""
    nb = len(gts_img)
    load(eng, df, n_raw, gts_img, keys_vals)
    s_img, f_img = eng.test_score_rows(seq[:, :nb])
    load(eng, df, n_raw, gts_scan, keys_vals)
    s_scan, f_scan = eng.test_score_rows(seq)
    return s_img.cpu().numpy(), f_img.cpu().numpy(), s_scan.cpu().numpy(), f_scan.cpu().numpy()


@pytest.fixture(scope='module')
def hand_runs(eng):
    seq, gts, names, closed = hand_batch(scan=True)
    nb = len(gts) - 1
    df = {}
    scorer = CR.CiderDOracle(df, N_RAW)
    ref = np.stack([oracle_scores(scorer, seq[c], gts) for c in range(2)])
    got = run_both_paths(eng, df, N_RAW, seq, gts[:nb], gts)
    return dict(seq=seq, gts=gts, names=names, closed=closed, nb=nb, ref=ref, got=got)


@pytest.fixture(scope='module')
def mixed_runs(eng):
    seq, gts_img, gts_scan, df, n = mixed_batch()
    scorer = CR.CiderDOracle(df, n)
    ref = np.stack([oracle_scores(scorer, seq[c], gts_scan) for c in range(2)])
    hits = order_hits(scorer, seq[0], gts_scan)
    got = run_both_paths(eng, df, n, seq, gts_img, gts_scan)
    return dict(seq=seq, gts=gts_scan, nb=len(gts_img), ref=ref, got=got, hits=hits, scorer=scorer)


def check_runs(r, names=None):
    s_img, f_img, s_scan, f_scan = r['got']
    nb, ref = r['nb'], r['ref']
    assert_rows(s_img, ref[:, :nb], names)
    assert_rows(s_scan, ref, names)
    assert close(f_img, 100.0 * ref[:, :nb].mean(1)).all(), (f_img, 100.0 * ref[:, :nb].mean(1))
    assert close(f_scan, 100.0 * ref.mean(1)).all(), (f_scan, 100.0 * ref.mean(1))


def test_hand_built_rows(hand_runs):
    """Case 1: chosen hypotheses (only the 0 token, no 0, L = 2-4, a token 16 times, a b a b, ids 1 / 8192 / 16383
    in n-grams one field apart) on both scorer kernels, every row against the oracle; the first four also
    against their closed forms."""
    r = hand_runs
    check_runs(r, r['names'])
    for i, c in enumerate(r['closed']):
        if c is not None:
            assert abs(r['ref'][0, i] - c) <= 1e-12 * max(1.0, c), (r['names'][i], r['ref'][0, i], c)
            for got in (r['got'][0], r['got'][2]):
                assert abs(got[0, i] - c) <= TOL * max(1.0, c), (r['names'][i], got[0, i], c)
    assert [c for c in r['closed'][:4]] == [10.0, 0.0, 2.5, 10.0]


@pytest.mark.parametrize('table', ['edges', 'empty', 'padded_100k'])
def test_df_edges(eng, table):
    """Case 2: the hand-built rows with df absent / 0.5 / 1 / 2 / N / 4 N on n-grams of both sides (a hypothesis whose
    unigram norm is exactly 0, one with negative weights on both sides); with an empty table; and with the table
    padded to 100 000 entries whose probe chains run off the end of the hash table and wrap."""
    import nicnes
    seq, gts, names, _ = hand_batch(scan=True)
    df, grams = edge_df()
    kv = None
    if table == 'empty':
        df = {}
    elif table == 'padded_100k':
        df_pad, tail = padded_df(df, grams)
        kv = nicnes.df_table_arrays(df_pad)
        cap = 64
        while cap < 2 * len(df_pad):
            cap <<= 1
        assert len(df_pad) == PAD_TOTAL and cap == PAD_CAP and tail > 48, (len(df_pad), cap, tail)
        with np.errstate(over='ignore'):
            slots = np_df_hash(np_keys(2, np.array([WRAP_PRESENT, WRAP_ABSENT]))) & np.uint64(PAD_CAP - 1)
            slots = slots.tolist() + (np_df_hash(np_keys(4, np.array([WRAP_LATE]))) & np.uint64(PAD_CAP - 1)).tolist()
        assert slots == [PAD_CAP - 1, PAD_CAP - 3, PAD_CAP - 1]
        assert df_pad[WRAP_PRESENT] == 2.0 and WRAP_ABSENT not in df_pad and df_pad[WRAP_LATE] == 2.0
    scorer = CR.CiderDOracle(df, N_RAW)     # the padding holds no n-gram of the rows: the same oracle values
    if table == 'edges':
        i, j = names.index('zero_weight_unigrams'), names.index('negative_weights')
        vec, norm, _ = scorer.counts2vec(CR.precook(CR.array_to_str(seq[0, i])))
        assert norm[0] == 0.0 and len(vec[0]) == 3 and norm[1] != 0.0
        vec, _, _ = scorer.counts2vec(CR.precook(CR.array_to_str(seq[0, j])))
        assert all(vec[0][(str(t),)] < 0 for t in (31, 32, 33))
        vr, _, _ = scorer.counts2vec(CR.precook(CR.array_to_str(gts[j][0])))
        assert all(vr[0][(str(t),)] < 0 for t in (31, 32, 33))
        assert set(df.values()) == {0.5, 1.0, 2.0, float(N_RAW), 4.0 * N_RAW} and len(df) < len(grams)
    ref = np.stack([oracle_scores(scorer, seq[c], gts) for c in range(2)])
    nb = len(gts) - 1
    got = run_both_paths(eng, df, N_RAW, seq, gts[:nb], gts, kv)
    check_runs(dict(got=got, nb=nb, ref=ref), names)
    assert np.array_equal(got[0], got[2][:, :nb])          # both kernels, bit for bit, on these tables too


def test_mixed_reference_counts(mixed_runs):
    """Case 3: 1 to 8 references per image (every column count of img_vr), a 464-row image table, and 1 / 8 / 9 / 20
    references in one batch on the scan path. Not vacuous: at least a third of the rows have a non-zero term of
    every n-gram order (from the oracle alone)."""
    r = mixed_runs
    counts = sorted(set(len(g) for g in r['gts'][:r['nb']]))
    assert counts == list(range(1, 9)) and sorted(set(len(g) for g in r['gts'])) == list(range(1, 10)) + [20]
    assert len(CR.precook(CR.array_to_str(r['gts'][64][0]))) == 58 and \
        len(all_ngrams(r['gts'][64])) == 464
    frac = r['hits'].mean(0)
    print('rows with a non-zero sim term per order:', frac.round(2).tolist())
    assert (frac >= 1.0 / 3.0).all(), frac
    assert (r['ref'][0] != 0).mean() > 0.9
    check_runs(r)


def test_both_kernels_agree_bit_for_bit(hand_runs, mixed_runs):
    """Case 7: the image-table kernel and the per-reference scan state the same arithmetic in the same order: the
    rows both paths scored are equal bit for bit."""
    for r in (hand_runs, mixed_runs):
        s_img, _, s_scan, _ = r['got']
        same = s_img == s_scan[:, :r['nb']]
        assert same.all(), [(tuple(i), s_img[tuple(i)].hex(), s_scan[tuple(i)].hex()) for i in np.argwhere(~same)[:8]]


# ---------------------------------------------------------------- case 4: launch geometry -----------
POOL = 1024


@pytest.fixture(scope='module')
def pool():
    """1024 images (1 to 8 references), 8 hypotheses each; the oracle scores of candidates 0 and 1 on every image
    and of all 8 on the first 33, computed once."""
    rng = np.random.Generator(np.random.PCG64(11))
    imgs = [gen_image(rng, int(rng.integers(1, 9)), 8) for _ in range(POOL)]
    nine = gen_image(rng, 9, 8)                          # stands in for the last image on the scan path
    gts = [i[0] for i in imgs]
    hyp = np.stack([np.stack([i[1][c] for i in imgs]) for c in range(8)])          # [8, POOL, T]
    df, n = CR.document_frequency_from_refs([strs(g) for g in gts + [nine[0]]])
    df = {tuple(int(w) for w in g): v for g, v in df.items()}
    scorer = CR.CiderDOracle(df, n)
    ref2 = np.stack([oracle_scores(scorer, hyp[c], gts) for c in range(2)])        # [2, POOL]
    ref8 = np.stack([oracle_scores(scorer, hyp[c, :33], gts[:33]) for c in range(8)])
    ref_nine = np.array([scorer.score_one(CR.array_to_str(nine[1][c]), strs(nine[0])) for c in range(2)])
    import nicnes
    return dict(gts=gts, hyp=hyp, df=df, n=n, kv=nicnes.df_table_arrays(df), ref2=ref2, ref8=ref8, nine=nine,
                ref_nine=ref_nine)


@pytest.mark.parametrize('B', [1, 3, 33, 130])
def test_geometry_eight_rows_per_workgroup(eng, pool, B):
    """Case 4: few candidates (8 rows per workgroup): one row, fewer rows than waves, B not a multiple of 8."""
    load(eng, None, pool['n'], pool['gts'][:B], pool['kv'])
    s, f = eng.test_score_rows(pool['hyp'][:2, :B])
    assert_rows(s.cpu().numpy(), pool['ref2'][:, :B])
    assert close(f.cpu().numpy(), 100.0 * pool['ref2'][:, :B].mean(1)).all()


def test_geometry_thirty_two_rows_per_workgroup(eng, pool):
    """Case 4: 1024 candidates x ceil(33 / 32) = 2048 workgroups: 32 rows per workgroup, the last one holding one
    row. The candidates are 8 distinct ones tiled in a scrambled order; every copy is asserted."""
    B = 33
    which = np.random.Generator(np.random.PCG64(12)).permutation(1024) % 8
    load(eng, None, pool['n'], pool['gts'][:B], pool['kv'])
    s, f = eng.test_score_rows(pool['hyp'][which, :B])
    assert s.shape == (1024, B)
    assert_rows(s.cpu().numpy(), pool['ref8'][which])
    assert close(f.cpu().numpy(), 100.0 * pool['ref8'][which].mean(1)).all()


@pytest.mark.parametrize('path', ['image_tables', 'scan'])
def test_geometry_largest_batch(eng, pool, path):
    """Case 4: B = 1024, the kernels' stated maximum (row_score[1024]), on both paths."""
    gts, hyp, ref = list(pool['gts']), pool['hyp'][:2].copy(), pool['ref2'].copy()
    if path == 'scan':
        gts[-1], hyp[:, -1], ref[:, -1] = pool['nine'][0], pool['nine'][1][:2], pool['ref_nine']
    load(eng, None, pool['n'], gts, pool['kv'])
    s, f = eng.test_score_rows(hyp)
    assert_rows(s.cpu().numpy(), ref)
    assert close(f.cpu().numpy(), 100.0 * ref.mean(1)).all()


# ---------------------------------------------------------------- case 5: batches and copies --------
def small_batches(seed, n_batches, B, rows_per_image, n_cand, max_k=8):
    rng = np.random.Generator(np.random.PCG64(seed))
    gts, hyps = [], []
    for _ in range(n_batches):
        ks = [max_k] + [int(k) for k in rng.integers(1, max_k + 1, B - 1)]
        imgs = [gen_image(rng, k, n_cand * rows_per_image) for k in ks]
        gts.append([i[0] for i in imgs])
        # [n_cand, B * rpi, T]: row b = copy b % rpi of image b // rpi
        hyps.append(np.stack([np.concatenate([i[1][c * rows_per_image:(c + 1) * rows_per_image] for i in imgs])
                              for c in range(n_cand)]))
    df, n = CR.document_frequency_from_refs([strs(g) for b in gts for g in b])
    return gts, hyps, {tuple(int(w) for w in g): v for g, v in df.items()}, n


@pytest.mark.parametrize('max_k', [8, 12], ids=['image_tables', 'scan'])
@pytest.mark.parametrize('n_batches,rpi', [(3, 1), (1, 3), (3, 3)], ids=['batches', 'copies', 'batches_and_copies'])
def test_batches_and_rows_per_image(eng, n_batches, rpi, max_k):
    """Case 5: candidates on their member's batch (member_batch [2, 0, 1, 2]) and / or three rows per image in a
    sampled mode (row b against image b // 3), against rollout_fitness(seq_per_img) on the right batch."""
    import nicnes
    B, mb = 5, ([2, 0, 1, 2] if n_batches > 1 else None)
    gts, hyps, df, n = small_batches(31 + rpi, n_batches, B, rpi, 8, max_k)
    scorer = CR.CiderDOracle(df, n)
    cand_batch = [mb[c // 2] if mb else 0 for c in range(8)]
    seq = np.stack([hyps[cand_batch[c]][c] for c in range(8)])
    eng.set_df_table(*nicnes.df_table_arrays(df), np.log(float(n)))
    eng.set_batches([(np.zeros((B, eng.cfg.fc_feat_size), np.float32), g) for g in gts])
    eng.set_fitness_mode('sample' if rpi > 1 else 'greedy')
    eng.set_rows_per_image(rpi)
    try:
        s, f = eng.test_score_rows(seq, member_batch=mb)
    finally:
        eng.set_fitness_mode('greedy')
        eng.set_rows_per_image(1)
    s, f = s.cpu().numpy(), f.cpu().numpy()
    assert s.shape == (8, B * rpi)
    for c in range(8):
        f_ref, sc_ref = CR.rollout_fitness(scorer, seq[c], gts[cand_batch[c]], seq_per_img=rpi)
        assert_rows(s[c], sc_ref)
        assert abs(f[c] - f_ref) <= TOL * max(1.0, abs(f_ref)), (c, f[c], f_ref)


# ---------------------------------------------------------------- case 6: criteria ------------------
LP_VALUES = np.array([0.0, -1e-3, -1.0, -20.0, -50.0], np.float32)


def criteria_case(rpi, max_k, sampled):
    """7 images, 2 candidates of 7 * rpi rows: tokens, log-probs from LP_VALUES, the oracle's row scores, and for the
    self-critical modes a baseline [n_cand, B] around each image's mean score (rewards of both signs)."""
    B, n_cand = 7, 2
    gts, hyps, df, n = small_batches(57, 1, B, rpi, n_cand, max_k)
    gts, seq = gts[0], hyps[0].copy()
    rows = B * rpi
    seq[:, 0] = row(0)                                     # first token 0: only step 0 counts
    seq[0, 1] = gts[1 // rpi][0]                           # a reference itself: a high score
    seq[:, 2] = row(*range(1, 17))                         # no 0 at all: every step counts
    seq[1, 3] = row(0)
    # the rows are shaped like a decode's: zeros from the first 0 on (finish_fitness stops a row's mask at its first
    # 0, which equals the reference's elementwise mask seq[t - 1] > 0 only on such rows)
    assert all((r[np.argmax(r == 0):] == 0).all() for r in seq.reshape(-1, T) if (r == 0).any())
    rng = np.random.Generator(np.random.PCG64(58))
    lp = LP_VALUES[rng.integers(0, len(LP_VALUES), (n_cand, rows, T))]
    lp[0, 1], lp[1, 2] = 0.0, -50.0
    scorer = CR.CiderDOracle(df, n)
    sc = np.stack([oracle_scores(scorer, seq[c], gts, rpi) for c in range(n_cand)])
    base = sc.reshape(n_cand, B, rpi).mean(2) * rng.uniform(0.0, 2.0, (n_cand, B)) + 0.01 if sampled else None
    reward = sc - np.repeat(base, rpi, 1) if sampled else sc
    if sampled:
        assert (reward < 0).sum() >= 3 and (reward > 0).sum() >= 3
    return B, n_cand, gts, seq, lp, df, n, sc, base, reward


@pytest.mark.parametrize('max_k', [8, 12], ids=['image_tables', 'scan'])
@pytest.mark.parametrize('mode,rpi', [('greedy_logprob', 1), ('greedy_expprob', 1), ('greedy_linprob', 1),
                                      ('greedy_avgprob', 1), ('sc_loss', 1), ('sc_loss', 2), ('self_critical', 1),
                                      ('self_critical', 2)])
def test_criteria_on_given_logprobs(eng, mode, rpi, max_k):
    """Case 6: the criteria on log-probs the decode never produces (0, -1e-3, -1, -20, -50), rows whose first token is
    0 (mask = the first step only), a row with no 0, and a baseline for the self-critical modes whose differences
    are negative on some rows."""
    sampled = mode in ('sc_loss', 'self_critical')
    B, n_cand, gts, seq, lp, df, n, sc, base, reward = criteria_case(rpi, max_k, sampled)
    load(eng, df, n, gts)
    eng.set_fitness_mode(mode)
    eng.set_rows_per_image(rpi)
    try:
        s, f = eng.test_score_rows(seq, lp=lp, base=base)
    finally:
        eng.set_fitness_mode('greedy')
        eng.set_rows_per_image(1)
    s, f = s.cpu().numpy(), f.cpu().numpy()
    assert_rows(s, sc)
    for c in range(n_cand):
        if mode == 'self_critical':
            want, tol = 100.0 * reward[c].mean(), TOL
        else:
            want, tol = CR.criterion_fitness(mode, lp[c], seq[c], reward[c]), TOL_CRIT
        assert abs(f[c] - want) <= tol * max(1.0, abs(want)), (mode, c, f[c], want)


# ---------------------------------------------------------------- case 8: no state leaks ------------
def dense_then_sparse():
    """4 dense images (8 references of 16 distinct tokens), then 4 sparse ones made of the dense image's own tokens:
    two with one reference (the first 6 tokens of dense reference 3), two with a 2-token and a 10-token reference
    (the long one's n-grams first appear in reference 1, so their reference-0 column of img_vr must read as 0).
    The hypotheses: dense references 0 and 1 (nothing in common with the sparse references: a stale table row
    would score), sparse references themselves, and dense reference 3."""
    rng = np.random.Generator(np.random.PCG64(91))
    dense = [dense_image(rng)[0] for _ in range(4)]
    sparse = [row(*d[3, :6], 0)[None] for d in dense[:2]] + \
             [np.stack([row(*d[4, :2], 0), row(*d[3, :10], 0)]) for d in dense[2:]]
    seq = np.stack([np.stack([d[c] for d in dense]) for c in range(2)])
    seq[0, 1], seq[1, 2], seq[1, 3] = sparse[1][0], dense[2][3], sparse[3][1]
    return dense, sparse, seq


def test_no_state_leaks_between_batches(eng):
    """Case 8: a dense 464-row batch, then a batch of 1- and 2-reference images on the same handle (img_vr memset,
    img_hkey rewrite): bit for bit the scores of a fresh handle that saw only the second batch. The second
    batch's hypotheses are mostly the first batch's references."""
    dense, sparse, seq = dense_then_sparse()
    df, n = CR.document_frequency_from_refs([strs(g) for g in dense + sparse])
    scorer = CR.CiderDOracle(df, n)
    load(eng, df, n, dense)
    s_dense = eng.test_score_rows(seq)[0].cpu().numpy()
    assert_rows(s_dense, np.stack([oracle_scores(scorer, seq[c], dense) for c in range(2)]))
    assert (s_dense > 0.0).all()                            # each hypothesis is (part of) one of the image's references
    eng.set_batch(np.zeros((4, eng.cfg.fc_feat_size), np.float32), sparse)
    s_after, f_after = eng.test_score_rows(seq)
    fresh = make_engine()
    try:
        load(fresh, df, n, sparse)
        s_fresh, f_fresh = fresh.test_score_rows(seq)
        assert torch.equal(s_after.cpu(), s_fresh.cpu()) and torch.equal(f_after.cpu(), f_fresh.cpu())
    finally:
        fresh.close()
    ref = np.stack([oracle_scores(scorer, seq[c], sparse) for c in range(2)])
    assert_rows(s_after.cpu().numpy(), ref)
    assert ref[0, 1] == pytest.approx(10.0) and 5.0 < ref[1, 3] < 5.1 and 0.0 < ref[1, 2] < 5.0
    assert ref[0, 0] == 0.0 and ref[0, 2] == 0.0 and ref[0, 3] == 0.0 and ref[1, 0] == 0.0 and ref[1, 1] == 0.0


def test_no_state_leaks_between_df_tables(eng):
    """Case 8: a df table replaced between two set_batch calls: the scores of a fresh handle that saw only the
    second table, bit for bit; and no scoring between set_df_table and the next set_batch."""
    import nicnes
    seq, gts, names, _ = hand_batch()
    df1, _ = edge_df()
    df2 = {g: (3.0 if v == 0.5 else 0.5 * v) for g, v in df1.items()}
    df2[(7,)] = 9.0
    load(eng, df1, N_RAW, gts)
    s1 = eng.test_score_rows(seq)[0].cpu()
    eng.set_df_table(*nicnes.df_table_arrays(df2), np.log(25.0))
    with pytest.raises(nicnes.NicnesError, match='nicnes_set_batch first'):
        eng.test_score_rows(seq)                            # the reference vectors are of the old table
    eng.set_batch(np.zeros((len(gts), eng.cfg.fc_feat_size), np.float32), gts)
    s2, f2 = eng.test_score_rows(seq)
    fresh = make_engine()
    try:
        load(fresh, df2, 25, gts)
        s_fresh, f_fresh = fresh.test_score_rows(seq)
        assert torch.equal(s2.cpu(), s_fresh.cpu()) and torch.equal(f2.cpu(), f_fresh.cpu())
    finally:
        fresh.close()
    assert not torch.equal(s1, s2.cpu())
    assert_rows(s2.cpu().numpy(), np.stack([oracle_scores(CR.CiderDOracle(df2, 25), seq[c], gts) for c in range(2)]),
                names)


# ---------------------------------------------------------------- case 9: the evaluate's scorer -----
@pytest.mark.parametrize('mode', ['greedy', 'greedy_logprob'])
def test_entry_is_the_evaluates_scorer(mode):
    """Case 9: an evaluate's own tokens and log-probs fed back through the entry give its fitness bit for bit."""
    import nicnes
    import nicnes.synthetic as S
    noise_len = 1 << 22
    e = nicnes.Engine(max_batch=16, max_members=2, noise_len=noise_len, noise_seed=5)
    try:
        S.setup_engine_workload(e, B=12, noise=S.noise_table(noise_len), df_sets=64)
        e.set_fitness_mode(mode)
        fit, seq, lp = e.evaluate(3, 0, 2, 0.01, return_seq=True, return_lp=True)
        s, f = e.test_score_rows(seq.reshape(4, 12, T), lp=lp.reshape(4, 12, T))
        assert torch.equal(f.cpu(), fit.reshape(4).cpu())
        assert len(set(fit.cpu().ravel().tolist()) - {0.0}) >= 2        # not four equal zeros
    finally:
        e.close()


# ---------------------------------------------------------------- case 10: seq_length 7 -------------
def test_seq_length_seven():
    """Case 10: the hand-built rows cut to 7 tokens on a seq_length = 7 handle (captions of 7 tokens without a 0)."""
    e = make_engine(seq_length=7)
    try:
        seq, gts, names, _ = hand_batch(7, scan=True)
        assert seq.shape[2] == 7 and CR.array_to_str(seq[0, names.index('abab')]) == '50 60 50 60 50 60 50'
        nb = len(gts) - 1
        for df in ({}, edge_df(7)[0]):
            scorer = CR.CiderDOracle(df, N_RAW)
            ref = np.stack([oracle_scores(scorer, seq[c], gts) for c in range(2)])
            got = run_both_paths(e, df, N_RAW, seq, gts[:nb], gts)
            check_runs(dict(got=got, nb=nb, ref=ref), names)
            assert np.array_equal(got[0], got[2][:, :nb])
    finally:
        e.close()


# ---------------------------------------------------------------- case 11: argument checks ----------
def test_argument_checks():
    """Case 11: every refusal of nicnes_test_score_rows, a good call afterwards, and set_batches' refusal of a
    reference token outside the vocabulary."""
    import nicnes
    e = make_engine(vocab=63, max_batch=8, max_members=2)
    try:
        B = 3
        gts = [np.stack([row(5, 6, 7, 0)]), np.stack([row(8, 9, 0), row(9, 8, 0)]), np.stack([row(63, 1, 0)])]
        fc = np.zeros((B, e.cfg.fc_feat_size), np.float32)
        seq = np.stack([np.stack([row(5, 6, 7, 0), row(8, 9, 0), row(1, 63, 0)])] * 2)
        with pytest.raises(nicnes.NicnesError, match='nicnes_set_batch first'):
            e.test_score_rows(seq)                                           # nothing set
        e.set_df_table(np.zeros(0, np.uint64), np.zeros(0), math.log(10.0))
        with pytest.raises(nicnes.NicnesError, match='nicnes_set_batch first'):
            e.test_score_rows(seq)                                           # a df table, no batch
        for bad in (64, -1):
            g = [x.copy() for x in gts]
            g[1][1, 1] = bad
            with pytest.raises(ValueError, match='reference token outside'):
                e.set_batch(fc, g)
        with pytest.raises(nicnes.NicnesError, match='nicnes_set_batch first'):
            e.test_score_rows(seq)                                           # the refused batches were not set
        e.set_batch(fc, gts)
        scorer = CR.CiderDOracle({}, 10)
        ref = np.stack([oracle_scores(scorer, seq[c], gts) for c in range(2)])

        def good(**kw):
            s, f = e.test_score_rows(seq, **kw)
            assert_rows(s.cpu().numpy(), ref)
            assert close(f.cpu().numpy(), 100.0 * ref.mean(1)).all()

        good()
        refusals = [
            dict(seq=seq[:, :2]),                                            # rows != B
            dict(seq=np.concatenate([seq, seq[:, :1]], 1)),
            dict(seq=np.concatenate([seq] * 3)[:5]),                         # n_cand 5 > 2 * max_members
            dict(seq=np.concatenate([seq] * 3)),                             # n_cand 6
            dict(seq=np.concatenate([seq, seq[:1]]), member_batch=[0, 0]),   # a member map with an odd n_cand
            dict(seq=seq, member_batch=[1]),                                 # one batch held: only batch 0
            dict(seq=seq, member_batch=[-1]),
        ]
        for kw in refusals:
            with pytest.raises(nicnes.NicnesError, match='invalid argument'):
                e.test_score_rows(**kw)
            good()
        e.set_fitness_mode('sample')
        e.set_rows_per_image(2)
        try:
            with pytest.raises(nicnes.NicnesError, match='rows must be'):
                e.test_score_rows(seq)                                       # rows != B * rpi in a sampled mode
            e.set_fitness_mode('greedy')                                     # rpi is 1 in the greedy modes
            good()
        finally:
            e.set_fitness_mode('greedy')
            e.set_rows_per_image(1)
        good(member_batch=[0])
        e.set_batches([(fc, gts), (fc, gts[::-1])])
        with pytest.raises(nicnes.NicnesError, match='several batches'):
            e.test_score_rows(seq)                                           # two batches held: the map is required
        with pytest.raises(nicnes.NicnesError, match='member_batch entry'):
            e.test_score_rows(seq, member_batch=[2])
        good(member_batch=[0])
    finally:
        e.close()
