"""GPU: the caption metrics on the device (vlp_caption_eval, csrc/caption_eval.hip) against the project's own host classes on word strings
(vlp_amd.scst.CiderD(df=table) and Bleu.sentence_stats, vlp_amd.caption_metrics.Rouge / lcs_len, all fp64 or exact).
tests/test_caption_metrics_cpu.py checks those classes; tests/caption_eval_util.py holds what the two files share.

(a) the kernel against the host classes on seeded corpora: bleu_stats and lcs exactly, cider within the bound.  Asserted on the host values
    alone, before any kernel output is read: for G >= 5 and T >= 21 at least half of the valid pairs have 0 < lcs < min(len_h, len_r), for
    G >= 64 at least one group has no reference that is both precision-best and recall-best;
(b) hand-built hard rows in one G = 8, R = 3, T = 64 case (caption_eval_util.hard_case says what each row is for); garbage behind a first 0
    and in invalid reference rows changes no bit of any output;
(c) the contract: strided rows with poisoned padding, guard bands around the three outputs and the workspace, bit-equal repeats, one capture
    into a graph replayed on new inputs, refusals by return code with nothing written;
(d) CaptionMetrics on="device" against on="host" (two chunk sizes, three images through the host fallback) and the command-line tool.

Bound on cider: the project's (4 T + 16) * 2^-24 * 10 of test_82 -- the arithmetic is vlp_cider_d_df's.  Every test prints what it measured
through report() (pytest -s); the figures of an MI355X run are in profiles/caption_eval.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import caption_eval_util as CU                           # noqa: E402
from tests import guard_util as GU                                  # noqa: E402
from vlp_amd import _lib as K                                       # noqa: E402
from vlp_amd import caption_metrics as CM                           # noqa: E402
from vlp_amd import eval_captions as EC                             # noqa: E402
from vlp_amd import scst as SC                                      # noqa: E402

DEV = torch.device("cuda:0")
REPORT = {}
bound = CU.bound


def report(key, **kw):
    """Prints what a test measured; with VLP_CAPTION_EVAL_RECORD=<json file> (profiles/caption_eval.json when the record is taken) the
    figures are also kept under that file's "test_85" key, next to the timing runs tools/caption_eval_bench.py writes there."""
    REPORT.setdefault(key, {}).update(kw)
    print("%s: %s" % (key, json.dumps(REPORT[key], sort_keys=True)))
    path = os.environ.get("VLP_CAPTION_EVAL_RECORD")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec.setdefault("test_85", {})[key] = REPORT[key]
        with open(path, "w") as f:
            json.dump(rec, f, indent=2, sort_keys=True)


def run_kernel(hyp, ref, count, tab):
    G, R, T = ref.shape
    h, r = torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV)
    c = torch.from_numpy(count).to(DEV) if count is not None else None
    keys, vals = tab.to(DEV)
    cider = torch.full((G,), float("nan"), device=DEV)
    stats = torch.full((G, 6), -7, dtype=torch.int32, device=DEV)
    lcs = torch.full((G, R, 2), -7, dtype=torch.int32, device=DEV)
    K.caption_eval(h, r, c, cider, stats, lcs, keys, vals, tab.n_docs)
    torch.cuda.synchronize()
    return cider.cpu(), stats.cpu(), lcs.cpu()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- (a) the kernel against the host classes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CU.SHAPES, ids=["G%d_R%d_T%d" % s for s in CU.SHAPES])
def test_kernel_against_host_classes(shape):
    G, R, T = shape
    seed = CU.seed_of(shape)
    hyp, ref, count = CU.make_corpus(G, R, T, seed)
    tab = CU.table(T)
    w_stats, w_lcs, w_cider, _ = CU.host_values(hyp, ref, count, tab, cache_key=(shape, seed))
    # asserted on the host values alone, before the kernel's output is looked at
    share, split = CU.lcs_shares(w_stats, w_lcs, count)
    if G >= 5 and T >= 21:
        assert share >= 0.5, share
    if G >= 64:
        assert split >= 1, split
    cider, stats, lcs = run_kernel(hyp, ref, count, tab)
    err = float(np.abs(cider.double().numpy() - w_cider).max())
    report("kernel_G%d_R%d_T%d" % shape, seed=seed, cider_max_abs_err=err, bound=bound(T), inner_lcs_share=share, split_best_groups=split,
           max_cider=float(w_cider.max()), empty_hypotheses=int((w_stats[:, 4] == 0).sum()), table_keys=len(tab))
    assert np.array_equal(stats.numpy(), w_stats)
    assert np.array_equal(lcs.numpy(), w_lcs)
    assert err <= bound(T), (err, bound(T))


# ---- (b) hand-built hard rows ---------------------------------------------------------------------------------------------------------
def test_hard_rows():
    G, R, T = 8, 3, 64
    hyp, ref, count = CU.hard_case(True)
    tab = CU.table(T)
    w_stats, w_lcs, w_cider, w_rouge = CU.host_values(hyp, ref, count, tab)
    # what the rows were built for, on the host values
    assert w_cider[0] == 0 and w_rouge[0] == 0
    assert w_stats[0].tolist() == [0, 0, 0, 0, 0, 5] and w_lcs[0].tolist() == [[0, 9], [0, 5], [0, 0]]
    assert not (hyp[1] == 0).any() and w_lcs[1].tolist() == [[64, 64], [63, 63], [0, 0]] and w_stats[1].tolist() == [64, 63, 62, 61, 64, 64]
    assert w_rouge[1] == 1.0 and abs(w_cider[1] - 10.0) < 2.0
    assert 0 < w_lcs[2, 0, 0] < 40 and w_stats[2, 0] == 64                       # reversed: every word found, a short common subsequence
    assert w_lcs[3].tolist() == [[10, 64], [3, 3], [0, 0]] and w_rouge[3] == 1.0   # precision from one reference, recall from the other
    assert w_lcs[4].tolist() == [[0, 15], [0, 0], [0, 0]] and w_stats[4, 0] == 0
    assert w_lcs[5].tolist() == [[2, 3], [0, 0], [0, 0]]
    assert w_lcs[6].tolist() == [[0, 0], [6, 7], [0, 0]] and w_stats[6, 5] == 7
    assert w_lcs[7].tolist()[0] == [63, 64] and w_lcs[7, 1, 1] == 63 and w_stats[7, 4] == 63
    cider, stats, lcs = run_kernel(hyp, ref, count, tab)
    err = float(np.abs(cider.double().numpy() - w_cider).max())
    report("hard_rows", cider_max_abs_err=err, bound=bound(T), host_cider=[round(float(v), 6) for v in w_cider], lcs=w_lcs[:, :, 0].tolist())
    assert np.array_equal(stats.numpy(), w_stats) and np.array_equal(lcs.numpy(), w_lcs)
    assert err <= bound(T), (err, bound(T))
    assert float(cider[0]) == 0.0 and float(cider[4]) == 0.0
    # garbage behind the first 0 and in invalid reference rows changes no bit
    hyp0, ref0, count0 = CU.hard_case(False)
    assert np.array_equal(count, count0) and not np.array_equal(ref, ref0) and not np.array_equal(hyp, hyp0)
    cider0, stats0, lcs0 = run_kernel(hyp0, ref0, count0, tab)
    assert same_bits(cider, cider0) and torch.equal(stats, stats0) and torch.equal(lcs, lcs0)
    # an empty table is legal: every df is 0
    empty = SC.DocFreq(tab.keys[:0], tab.vals[:0], tab.n_docs)
    cider_e, stats_e, lcs_e = run_kernel(hyp, ref, count, empty)
    assert torch.equal(stats_e, stats) and torch.equal(lcs_e, lcs)
    assert float(np.abs(cider_e.double().numpy() - CU.host_cider(hyp, ref, count, empty)).max()) <= bound(T)


# ---- (c) contract ---------------------------------------------------------------------------------------------------------------------
def _guarded_table(tab):
    gk = GU.guarded_vec(len(tab), dtype=torch.int64, fill=CU.U.key_of((1000,)), device=DEV)        # guards: a real key
    gk.vec.copy_(torch.from_numpy(tab.keys.view(np.int64)).to(DEV))
    gv = GU.guarded_vec(len(tab), dtype=torch.int32, fill=7, device=DEV)
    gv.vec.copy_(torch.from_numpy(tab.vals).to(DEV))
    return gk.seal(), gv.seal()


def test_contract_guards_strides_and_determinism():
    G, R, T = 5, 3, 21
    hyp, ref, count = CU.make_corpus(G, R, T, CU.seed_of((G, R, T)))
    tab = CU.table(T)
    plain = run_kernel(hyp, ref, count, tab)
    # rows with strides larger than T; the padding and the guards hold 1000, a real word
    gh = GU.guarded(G, T, ld=T + 5, dtype=torch.int64, fill=1000, device=DEV).set(torch.from_numpy(hyp).to(DEV))
    gr = GU.guarded(G * R, T, ld=T + 3, dtype=torch.int64, fill=1000, device=DEV).set(torch.from_numpy(ref.reshape(G * R, T)).to(DEV))
    gc = GU.guarded_vec(G, dtype=torch.int32, fill=R, device=DEV)
    gc.vec.copy_(torch.from_numpy(count).to(DEV))
    gc.seal()
    gk, gv = _guarded_table(tab)
    ref_view = gr.full.view(G, R, T + 3)[:, :, :T]
    assert ref_view.stride() == (R * (T + 3), T + 3, 1) and gh.view.stride() == (T + 5, 1)
    need = K.caption_eval_workspace_bytes(G, R, T)
    assert need == K.cider_d_df_workspace_bytes(G, R, T, 1) > 0
    outs = []
    for _ in range(2):
        gs = GU.guarded_vec(G, dtype=torch.float32, fill="sentinel", device=DEV)
        gb = GU.guarded_vec(G * 6, dtype=torch.int32, fill="sentinel", device=DEV)
        gl = GU.guarded_vec(G * R * 2, dtype=torch.int32, fill="sentinel", device=DEV)
        ws = GU.guarded_vec(need, dtype=torch.uint8, fill="sentinel", device=DEV)
        K.caption_eval(gh.view, ref_view, gc.vec, gs.vec, gb.vec, gl.vec, gk.vec, gv.vec, tab.n_docs, workspace=ws.vec)
        torch.cuda.synchronize()
        for g, name, written in ((gs, "cider", "logical"), (gb, "bleu_stats", "logical"), (gl, "lcs", "logical"), (ws, "workspace", "logical"),
                                 (gh, "hyp", None), (gr, "ref", None), (gc, "ref_count", None), (gk, "df_keys", None), (gv, "df_vals", None)):
            GU.assert_untouched(g, written=written, name=name)
        for g, name in ((gs, "cider"), (gb, "bleu_stats"), (gl, "lcs")):
            GU.assert_written(g, name=name)
        outs.append((gs.vec.clone().cpu(), gb.vec.clone().cpu().view(G, 6), gl.vec.clone().cpu().view(G, R, 2)))
    for a, b in ((outs[0], outs[1]), (outs[0], plain)):
        assert same_bits(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # ref_count = NULL means all R
    all_r = run_kernel(hyp, ref, None, tab)
    full = run_kernel(hyp, ref, np.full(G, R, dtype=np.int32), tab)
    assert same_bits(all_r[0], full[0]) and torch.equal(all_r[1], full[1]) and torch.equal(all_r[2], full[2])
    w_stats, w_lcs, w_cider, _ = CU.host_values(hyp, ref, None, tab)
    assert np.array_equal(full[1].numpy(), w_stats) and np.array_equal(full[2].numpy(), w_lcs)
    assert float(np.abs(full[0].double().numpy() - w_cider).max()) <= bound(T)


def test_capture_into_a_graph_and_replay_on_new_inputs():
    G, R, T = 16, 5, 21
    tab = CU.table(T)
    keys, vals = tab.to(DEV)
    hyp, ref, count = CU.make_corpus(G, R, T, 0)
    h, r, c = torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV), torch.from_numpy(count).to(DEV)
    cider = torch.zeros(G, device=DEV)
    stats = torch.zeros((G, 6), dtype=torch.int32, device=DEV)
    lcs = torch.zeros((G, R, 2), dtype=torch.int32, device=DEV)
    ws = torch.empty(K.caption_eval_workspace_bytes(G, R, T), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.caption_eval(h, r, c, cider, stats, lcs, keys, vals, tab.n_docs, workspace=ws)              # warm-up: code objects loaded
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                                                       # any synchronising call fails the capture
        K.caption_eval(h, r, c, cider, stats, lcs, keys, vals, tab.n_docs, workspace=ws)
    hyp2, ref2, count2 = CU.make_corpus(G, R, T, 3)
    assert not np.array_equal(hyp, hyp2)
    h.copy_(torch.from_numpy(hyp2))
    r.copy_(torch.from_numpy(ref2))
    c.copy_(torch.from_numpy(count2))
    graph.replay()
    torch.cuda.synchronize()
    w_stats, w_lcs, w_cider, _ = CU.host_values(hyp2, ref2, count2, tab)
    assert not np.array_equal(w_stats, CU.host_counts(hyp, ref, count)[0])
    err = float(np.abs(cider.double().cpu().numpy() - w_cider).max())
    report("graph_replay", cider_max_abs_err=err, bound=bound(T))
    assert np.array_equal(stats.cpu().numpy(), w_stats) and np.array_equal(lcs.cpu().numpy(), w_lcs) and err <= bound(T)


REFUSALS = ["T65", "R9", "G1025", "G0", "mult2", "reward", "stats_null", "lcs_null", "workspace_short", "df_n_negative", "n_docs_0", "n_docs_above_2p24",
            "keys_null", "vals_null", "keys_misaligned", "vals_misaligned"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_by_return_code(what):
    G, R, T = {"T65": (2, 1, 65), "R9": (2, 9, 4), "G1025": (1025, 1, 4), "G0": (0, 1, 4)}.get(what, (2, 2, 4))
    mult = 2 if what == "mult2" else 1
    hyp = torch.full((max(mult * G, 1), T), 1000, dtype=torch.int64, device=DEV)[:mult * G]
    ref = torch.full((max(G, 1), R, T), 1000, dtype=torch.int64, device=DEV)[:G]
    tab = CU.table(4)
    gk, gv = _guarded_table(tab)
    gs = GU.guarded_vec(max(mult * G, 1), dtype=torch.float32, fill="sentinel", device=DEV)
    gw = GU.guarded_vec(max(G, 1), dtype=torch.float32, fill="sentinel", device=DEV)
    gb = GU.guarded_vec(max(G, 1) * 6, dtype=torch.int32, fill="sentinel", device=DEV)
    gl = GU.guarded_vec(max(G, 1) * R * 2, dtype=torch.int32, fill="sentinel", device=DEV)
    need = K.caption_eval_workspace_bytes(G, R, T)
    if what in ("T65", "R9", "G1025", "G0"):
        assert need == 0
    else:
        assert need > 0                                                   # the shape itself is fine: the same call without the fault runs
        K.caption_eval(hyp[:G], ref, None, gs.vec, gb.vec, gl.vec, gk.vec, gv.vec, tab.n_docs, workspace=torch.empty(need, dtype=torch.uint8, device=DEV))
        torch.cuda.synchronize()
        GU.assert_written(gb, name="bleu_stats")
        for g in (gs, gb, gl):
            g.fill_all("sentinel")
            g.seal()
    ws = GU.guarded_vec(max(need - 1, 16) if what == "workspace_short" else max(need, 4096), dtype=torch.uint8, fill="sentinel", device=DEV)
    if what == "workspace_short":
        assert ws.vec.numel() == need - 1
    s = K.CiderDArgs(K.ptr(hyp), hyp.stride(0), K.ptr(ref), ref.stride(0), ref.stride(1), None, G, R, T, mult, 6.0, K.ptr(gs.vec),
                     K.ptr(gw.vec) if what == "reward" else None, K.ptr(ws.vec), ws.vec.numel())
    kp, vp, n, n_docs = gk.vec.data_ptr(), gv.vec.data_ptr(), len(tab), tab.n_docs
    assert kp % 8 == 0 and vp % 4 == 0
    if what == "df_n_negative":
        n = -1
    elif what == "n_docs_0":
        n_docs = 0
    elif what == "n_docs_above_2p24":
        n_docs = 2 ** 24 + 1
    elif what == "keys_null":
        kp = None
    elif what == "vals_null":
        vp = None
    elif what == "keys_misaligned":
        kp, n = kp + 4, n - 1
    elif what == "vals_misaligned":
        vp, n = vp + 2, n - 1
    d = K.CiderDDfArgs(s, C.c_void_p(kp), C.c_void_p(vp), n, n_docs)
    a = K.CaptionEvalArgs(d, None if what == "stats_null" else K.ptr(gb.vec), None if what == "lcs_null" else K.ptr(gl.vec))
    rc = K.load().vlp_caption_eval(C.byref(a), K.stream_ptr())
    assert rc == -1, rc
    assert "vlp_caption_eval" in K.load().vlp_last_error_string().decode()
    torch.cuda.synchronize()
    for g, name in ((gs, "cider"), (gw, "reward"), (gb, "bleu_stats"), (gl, "lcs"), (ws, "workspace"), (gk, "df_keys"), (gv, "df_vals")):
        GU.assert_untouched(g, written=None, name=name)             # nothing was launched


# ---- (d) CaptionMetrics and the command-line tool -----------------------------------------------------------------------------------------
def test_caption_metrics_device_against_host():
    G, R, T = 300, 5, 21
    hyp, ref, count = CU.make_corpus(G, R, T, 0)
    refs, hyps = CU.word_lists(hyp, ref, count)
    rng = np.random.RandomState(11)
    hyps[17] = [int(w) for w in rng.randint(1000, 1012, size=70)]                       # a hypothesis of 70 words
    refs[130][0] = [int(w) for w in rng.randint(1000, 1012, size=65)]                   # a reference of 65 words
    refs[299] = [[int(w) for w in rng.randint(1000, 1012, size=rng.randint(3, 15))] for _ in range(9)]      # nine references
    host = CM.CaptionMetrics().score(refs, hyps, on="host")
    assert host["scored_on_host"] == 3
    fits = np.ones(G, dtype=bool)
    fits[[17, 130, 299]] = False
    for chunk in (128, 1024):
        dev = CM.CaptionMetrics(chunk=chunk, device=DEV).score(refs, hyps, on="device")
        assert dev["scored_on_host"] == 3 and dev["images"] == G
        for k in CM.METRICS[:5]:
            assert dev[k] == host[k], (k, dev[k], host[k])                               # equal as fp64 values
        assert np.array_equal(dev["per_image"]["bleu_stats"], host["per_image"]["bleu_stats"])
        assert np.array_equal(dev["per_image"]["ROUGE_L"], host["per_image"]["ROUGE_L"])
        err = np.abs(dev["per_image"]["CIDEr"] - host["per_image"]["CIDEr"])
        report("caption_metrics_chunk%d" % chunk, cider_max_abs_err=float(err.max()), bound=bound(T), corpus_cider_err=abs(dev["CIDEr"] - host["CIDEr"]),
               host={k: host[k] for k in CM.METRICS})
        assert float(err[fits].max()) <= bound(T) and float(err[~fits].max()) == 0.0     # the fallback is the host path itself
        assert abs(dev["CIDEr"] - host["CIDEr"]) <= bound(T)


def test_cli_device_against_host(tmp_path):
    src, prd, ids = CU.write_cli_case(tmp_path)
    base = ["--predictions", prd, "--src_file", src, "--split", "val", "--dataset", "coco"]
    per = {}
    out = {}
    for on in ("host", "device"):
        pf = os.path.join(tmp_path, "per_%s.json" % on)
        out[on] = EC.main(base + ["--metrics_on", on, "--per_image_file", pf])
        per[on] = json.load(open(pf))
    assert out["host"]["scored_on_host"] == 2 and out["device"]["scored_on_host"] == 2 and out["device"]["images"] == 7
    for k in CM.METRICS[:5]:
        assert out["device"][k] == out["host"][k], k
    b = bound(12)                                                                        # references of 5..11 words, captions of at most 10
    errs = [abs(a["CIDEr"] - c["CIDEr"]) for a, c in zip(per["device"], per["host"])]
    report("cli", cider_max_abs_err=max(errs), bound=b, host=out["host"])
    assert [a["image_id"] for a in per["device"]] == ids and max(errs) <= b and abs(out["device"]["CIDEr"] - out["host"]["CIDEr"]) <= b
    assert all(a["bleu_stats"] == c["bleu_stats"] and a["ROUGE_L"] == c["ROUGE_L"] for a, c in zip(per["device"], per["host"]))
