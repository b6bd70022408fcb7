"""GPU: duplicate n-gram blocking on the device (vlp_ngram_candidates, vlp_logsoftmax_topk_list, Engine.decode_beam(ngram=...)).

  * the candidates kernel against a host restatement of the reference's get_dup_ngram_candidates (modeling.py:1391-1406) on synthetic frames,
    at every frame, with guard bands around both outputs;
  * the list form of the top-k kernel against the dense-mask form (vlp_logsoftmax_topk) on the mask scattered from the same lists: integer
    ids and the scores' bit patterns must be equal -- there is no tolerance, both evaluate the same fp32 expression per element;
  * the decoder end to end: ngram_blocking="device" against "host" on the same model -- both launch the same model kernels on the same inputs,
    so every returned tensor must be equal -- over the first run, the graph capture and the replay, without any host blocker being built.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from oracle import vlp_oracle as O                         # noqa: E402  (checker: parameter init only)
from oracle.make_golden import decode_inputs               # noqa: E402  (pure helper)
from tests.guard_util import guarded, guarded_vec, assert_untouched, assert_written, bits   # noqa: E402
from vlp_amd import _lib as K                              # noqa: E402
from vlp_amd import synthetic as S                         # noqa: E402
from vlp_amd.modeling import BertConfig, BertForSeq2SeqDecoder   # noqa: E402

DEV = torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------
# vlp_ngram_candidates
# ------------------------------------------------------------------------------------------------
def host_candidates(seq, n, ignore):
    """get_dup_ngram_candidates (modeling.py:1391-1406), restated."""
    if len(seq) < n:
        return []
    tail = seq[-(n - 1):]
    if ignore and any(t in ignore for t in tail):
        return []
    cands = set()
    for i in range(len(seq) - (n - 1)):
        if seq[i:i + n - 1] == tail and not (ignore and seq[i + n - 1] in ignore):
            cands.add(seq[i + n - 1])
    return sorted(cands)


def host_sequences(wids, ptrs, s):
    """The hypotheses of frame s, row r = b*K + k, by following the back pointers (modeling.py:1376-1389)."""
    F, B, Kb = wids.shape
    out = []
    for b in range(B):
        for k in range(Kb):
            j, seq = k, []
            for f in range(s, -1, -1):
                seq.append(int(wids[f, b, j]))
                j = int(ptrs[f, b, j])
            out.append(seq[::-1])
    return out


B_, K_, F_ = 3, 4, 14
POOL5 = [7, 5003, 12001, 20011, 28995]          # 5 distinct ids spread over [0, 28996)
POOL3 = [7, 12001, 28995]


def synthetic_frames(pool, seed=0):
    g = torch.Generator().manual_seed(seed)
    wids = torch.tensor(pool)[torch.randint(0, len(pool), (F_, B_, K_), generator=g)]
    ptrs = torch.randint(0, K_, (F_, B_, K_), generator=g)
    ptrs[0] = 0
    return wids.contiguous(), ptrs.contiguous()


def run_candidates(wids, ptrs, n, ignore):
    """The kernel at every frame -> {s: [sorted list per row]}; checks counts' range and the write footprint on the way."""
    wd, pd = wids.to(DEV), ptrs.to(DEV)
    ign = torch.tensor(sorted(ignore), device=DEV, dtype=torch.long) if ignore else None
    rows = B_ * K_
    got = {}
    for s in range(F_):
        C = s + 1                                                     # the smallest row stride the ABI allows
        gi = guarded(rows, C, dtype=torch.int32, fill="sentinel", device=DEV)
        gc = guarded_vec(rows, dtype=torch.int32, fill="sentinel", device=DEV)
        K.ngram_candidates(wd, pd, B_, K_, s, n, gi.full, gc.vec, ignore_ids=ign)
        torch.cuda.synchronize()
        assert_written(gc, "logical", "cand_cnt")
        assert_untouched(gc, "logical", "cand_cnt")
        cnt = gc.vec.cpu()
        assert int(cnt.min()) >= 0 and int(cnt.max()) <= C, cnt
        foot = torch.arange(C, device=DEV).unsqueeze(0) < gc.vec.unsqueeze(1)
        assert_untouched(gi, foot, "cand_ids")                        # nothing past the first cnt entries of a row, nothing outside the rows
        assert_written(gi, foot, "cand_ids")
        ids = gi.full.cpu()
        got[s] = [sorted(ids[r, :int(cnt[r])].tolist()) for r in range(rows)]
        for r in range(rows):
            assert len(set(got[s][r])) == len(got[s][r]), "row %d frame %d: ids not distinct: %s" % (r, s, got[s][r])
    return got


@pytest.mark.parametrize("pool,n", [(POOL5, 2), (POOL5, 3), (POOL3, 4)])
def test_ngram_candidates_vs_host(pool, n):
    wids, ptrs = synthetic_frames(pool)
    ignore = {pool[2]}
    want = {ig: {s: [host_candidates(sq, n, ignore if ig else None) for sq in host_sequences(wids, ptrs, s)] for s in range(F_)} for ig in (False, True)}
    pairs = F_ * B_ * K_
    nonempty = sum(bool(c) for s in range(F_) for c in want[False][s])
    changed = sum(a != b for s in range(F_) for a, b in zip(want[False][s], want[True][s]))
    print("n=%d pool=%d: %d of %d (frame, row) pairs non-empty, the ignore set changes %d rows" % (n, len(pool), nonempty, pairs, changed))
    assert nonempty >= 0.1 * pairs and changed >= 1, "the recipe would pass vacuously"
    for s in range(n - 1):                                            # s + 1 < n: every count is 0
        assert not any(want[False][s])
    for ig in (False, True):
        got = run_candidates(wids, ptrs, n, ignore if ig else None)
        for s in range(F_):
            assert got[s] == want[ig][s], "n=%d ignore=%s frame %d:\n got %s\nwant %s" % (n, ig, s, got[s], want[ig][s])


def test_ngram_candidates_rejects_bad_arguments():
    wids, ptrs = [t.to(DEV) for t in synthetic_frames(POOL5)]
    ci = torch.zeros(B_ * K_, 8, dtype=torch.int32, device=DEV)
    cc = torch.zeros(B_ * K_, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        K.ngram_candidates(wids, ptrs, B_, K_, 8, 2, ci, cc)          # row stride 8 < s + 1 = 9
    with pytest.raises(RuntimeError):
        K.ngram_candidates(wids, ptrs, B_, K_, 3, 1, ci, cc)          # n = 1 is not a kernel case
    assert int(ci.abs().sum()) == 0 and int(cc.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------
# vlp_logsoftmax_topk_list == vlp_logsoftmax_topk on the scattered mask
# ------------------------------------------------------------------------------------------------
ROWS, CAND_LD = 6, 16
COUNTS = [0, 1, 3, 5, 8, 12]
EOS_ROW = 3                                     # this row's list holds eos_id (its unforbidden top-2 word)


def topk_case(V):
    """Logits whose best 24 words per row are planted above the random floor, with exact ties among them (three equal maxima, pairs further
    down), so that which words are forbidden and the index order inside a tie both decide the result."""
    g = torch.Generator().manual_seed(V)
    ld = (V + 63) // 64 * 64
    x = torch.randn(ROWS, ld, generator=g)
    x[:, V:] = 100.0                                                  # the ld padding must be ignored
    planted = torch.stack([torch.randperm(V, generator=g)[:24] for _ in range(ROWS)])
    vals = torch.tensor([8.0, 8.0, 8.0, 7.5, 7.5, 7.25, 7.0, 7.0, 6.75, 6.5, 6.5, 6.5] + [6.25 - 0.125 * (i // 2) for i in range(12)])
    x.scatter_(1, planted, vals.unsqueeze(0).expand(ROWS, -1).contiguous())
    x = x.half()
    top = torch.topk(x[:, :V].float(), 4, dim=1).indices              # any order inside the tie: all three maxima get listed
    cand = torch.empty(ROWS, CAND_LD, dtype=torch.int32)
    for r, c in enumerate(COUNTS):
        # what lies past the count must be ignored: fill it with a word whose blocking would change the row's result
        cand[r] = int(top[r, min(c, 3)])
        head = top[r, :min(c, 3)].tolist()
        rest = [v for v in torch.randperm(V, generator=g).tolist() if v not in head][:c - len(head)]
        cand[r, :c] = torch.tensor(head + rest, dtype=torch.int32)
    eos = int(top[EOS_ROW, 1])
    assert eos in cand[EOS_ROW, :COUNTS[EOS_ROW]].tolist()
    cnt = torch.tensor(COUNTS, dtype=torch.int32)
    forbid = torch.zeros(ROWS, V, dtype=torch.uint8)
    for r, c in enumerate(COUNTS):
        forbid[r, cand[r, :c].long()] = 1
    return x.to(DEV), ld, cand.to(DEV), cnt.to(DEV), forbid.to(DEV), eos


@pytest.mark.parametrize("V,Kb", [(28996, 3), (28996, 5), (28996, 16), (28996, 20), (1003, 5)])
def test_topk_list_equals_dense_mask(V, Kb):
    x, ld, cand, cnt, forbid, eos = topk_case(V)
    assert ld % 8 == 0
    for block in (False, True):
        ref_s = torch.zeros(ROWS, Kb, dtype=torch.float32, device=DEV)
        ref_i = torch.zeros(ROWS, Kb, dtype=torch.long, device=DEV)
        K.logsoftmax_topk(x, ld, ROWS, V, Kb, ref_s, ref_i, forbid=forbid, eos_id=eos, block_eos=block)
        gs = guarded(ROWS, Kb, dtype=torch.float32, fill="sentinel", device=DEV)
        gi = guarded(ROWS, Kb, dtype=torch.int64, fill="sentinel", device=DEV)
        K.logsoftmax_topk_list(x, ld, ROWS, V, Kb, gs.view, gi.view, cand, cnt, eos_id=eos, block_eos=block)
        torch.cuda.synchronize()
        assert_untouched(gs, "logical", "scores")
        assert_untouched(gi, "logical", "ids")
        assert torch.equal(gi.view, ref_i), (block, gi.view, ref_i)
        assert torch.equal(bits(gs.view), bits(ref_s)), (block, gs.view, ref_s)
        if not block:       # the case is not vacuous: every row that has a list lists its best word, so blocking changes its selection
            plain_i = torch.zeros(ROWS, Kb, dtype=torch.long, device=DEV)
            K.logsoftmax_topk(x, ld, ROWS, V, Kb, torch.zeros_like(ref_s), plain_i, eos_id=eos, block_eos=False)
            for r, c in enumerate(COUNTS):
                assert (c == 0) == torch.equal(plain_i[r], ref_i[r]), (r, plain_i[r], ref_i[r])


def test_topk_list_rejects_bad_arguments():
    x, ld, cand, cnt, forbid, eos = topk_case(1003)
    sc = torch.zeros(ROWS, 5, dtype=torch.float32, device=DEV)
    ids = torch.zeros(ROWS, 5, dtype=torch.long, device=DEV)
    wide = torch.zeros(ROWS, 1025, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        K.logsoftmax_topk_list(x, ld, ROWS, 1003, 5, sc, ids, wide, cnt)          # row stride above the kernel's list capacity


# ------------------------------------------------------------------------------------------------
# end to end: device blocking == host blocking
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decoder():
    p = O.init_params(vocab_size=1024, layers=2, tasks="img2txt", seed=27, std=0.1)            # the beam_2l_K3 model
    cfg = BertConfig(1024, num_hidden_layers=2, type_vocab_size=6)
    m = BertForSeq2SeqDecoder(cfg, mask_word_id=S.MASK_ID, eos_id=S.SEP_ID, enable_butd=True, len_vis_input=100, length_penalty=0.4)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    m.load_state_dict(sd, strict=True)
    return m.half().to(DEV).eval()


def run_search(m, inp, **attrs):
    for k, v in attrs.items():
        setattr(m, k, v)
    img, vis_pe, input_ids, token_type, pos, am = inp
    tr = m(img.half(), vis_pe.half(), input_ids, token_type, pos, am, task_idx=None)
    torch.cuda.synchronize()
    return tr


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("pred_seq", "wids", "ptrs", "scores"))


def test_decoder_has_the_blocking_switch():
    assert BertForSeq2SeqDecoder.ngram_blocking == "device"


@pytest.mark.parametrize("Kb,n,T,min_len,with_ignore", [(3, 2, 10, 2, False), (4, 3, 16, 0, False), (3, 2, 10, 2, True)])
def test_device_blocking_equals_host_blocking(decoder, monkeypatch, Kb, n, T, min_len, with_ignore):
    m = decoder
    inp = [t.to(DEV) for t in decode_inputs(3, T, 213)]
    base = dict(search_beam_size=Kb, ngram_size=n, min_len=min_len, forbid_ignore_set=None)
    if with_ignore:
        free = run_search(m, inp, forbid_duplicate_ngrams=False, **base)
        base["forbid_ignore_set"] = {int(free["pred_seq"][0, 0])}      # the first word of sample 0's unblocked best sequence

    def no_host_blocker(*a, **kw):
        raise AssertionError("the device path built the host n-gram blocker")
    devs, seen_ignore = [], []
    launch = K.ngram_candidates

    def spy(*a, **kw):                  # what the engine hands to the candidates kernel as the ignore list (python-side launches: plain run and capture)
        ign = kw.get("ignore_ids")
        seen_ignore.append(None if ign is None else ign.tolist())
        return launch(*a, **kw)
    with monkeypatch.context() as mp:
        mp.setattr(BertForSeq2SeqDecoder, "_ngram_blocker", no_host_blocker)
        mp.setattr(K, "ngram_candidates", spy)
        # the device path goes first.  The first two parametrisations meet a fresh workspace: plain run, graph capture, replay.  The ignore case
        # shares the workspace of the first one (module-scoped decoder, same key) and has run the unblocked search: capture, replay, replay.
        for rep in range(3):
            devs.append(run_search(m, inp, forbid_duplicate_ngrams=True, ngram_blocking="device", **base))
    assert seen_ignore, "the device path never launched the candidates kernel from python"
    want_ignore = sorted(base["forbid_ignore_set"]) if with_ignore else None
    assert all(ig == want_ignore for ig in seen_ignore), (seen_ignore[:3], want_ignore)     # the ignore list reaches the kernel as given
    host = run_search(m, inp, forbid_duplicate_ngrams=True, ngram_blocking="host", **base)
    free = run_search(m, inp, forbid_duplicate_ngrams=False, **base)
    for rep, dev in enumerate(devs):
        assert same(dev, host), "call %d: device and host blocking differ\n%s\n%s" % (rep, dev["pred_seq"], host["pred_seq"])
    differs = [not torch.equal(host["pred_seq"][b], free["pred_seq"][b]) for b in range(3)]
    print("samples whose blocked sequence differs from the unblocked one:", differs)
    assert any(differs), "blocking was never active: the comparison shows nothing"
    if with_ignore:
        plain = run_search(m, inp, forbid_duplicate_ngrams=True, ngram_blocking="device", **dict(base, forbid_ignore_set=None))
        print("ignore set changes the result:", not same(plain, host))
    with pytest.raises(ValueError):
        run_search(m, inp, forbid_duplicate_ngrams=True, ngram_blocking="gpu", **base)
    m.ngram_blocking = "device"


def test_ngram_size_one_stays_on_the_host(decoder, monkeypatch):
    """ngram_size == 1 keeps the host closure (the reference's seq[-0:] quirk is not a kernel case)."""
    called = []
    orig = BertForSeq2SeqDecoder._ngram_blocker

    def spy(self, *a, **kw):
        called.append(1)
        return orig(self, *a, **kw)
    monkeypatch.setattr(BertForSeq2SeqDecoder, "_ngram_blocker", spy)
    inp = [t.to(DEV) for t in decode_inputs(3, 6, 213)]
    run_search(decoder, inp, search_beam_size=3, ngram_size=1, min_len=0, forbid_ignore_set=None, forbid_duplicate_ngrams=True, ngram_blocking="device")
    assert called
