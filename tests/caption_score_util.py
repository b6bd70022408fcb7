"""Shared by tests/test_caption_score_cpu.py and tests/test_48_caption_score_gpu.py: the torch restatement of vlp_token_score's integer
outputs (include/vlp_hip.h), the hand-built rows of the kernel test, and the fixture of the tool test (tests/test_42_decode_cli_gpu.py's
recipe: 5 images in a packed store, a 2-layer checkpoint, a generated vocabulary) with a token file of given captions."""
import json
import os

import numpy as np
import torch

from tests import scst_policy_util as PU

NV, T, VOCAB = 100, 10, 1024
# 7 images over two splits; the 5 of "test" are in the store (in another order than the list's)
LIST = [("test", 391895), ("val", 522418), ("test", 184613), ("test", 318219), ("val", 554625), ("test", 574769), ("test", 60623)]


def rank_top_reference(rows16, ids):
    """From fp16 rows [R, V] and ids [R] (>= 0; clamped to V - 1): rank [R] = #{v: l_v > l_id} + #{v < id: l_v == l_id}, top_id [R] = the
    smallest column holding the row's maximum, top_logit [R] f32 = that maximum.  Integer / exact comparisons on the fp16 values as fp32."""
    x = rows16.detach().float().cpu()
    R, V = x.shape
    i = ids.detach().cpu().clamp(max=V - 1).view(R, 1)
    lid = x.gather(1, i)
    col = torch.arange(V).view(1, V)
    rank = ((x > lid) | ((x == lid) & (col < i))).sum(1)
    top = x.max(1).values
    top_id = torch.where(x == top.view(R, 1), col.expand(R, V), torch.full((R, V), V)).min(1).values
    return rank.to(torch.int32), top_id, top


def hard_score_rows(V=1000):
    """name -> (fp16 row [V], id, expected rank or None, expected top_id or None): the rows of the issue with the values they must give."""
    rows = {}
    for name, (row, id) in PU.hard_rows(V).items():
        rows[name] = (row, id, None, None)
    rows["all_equal"] = rows["all_equal"][:2] + (V // 2, 0)                 # rank = id, top_id = 0
    gen = torch.Generator().manual_seed(9)
    x = (torch.randn(V, generator=gen) * 2.0).half()
    tied = x.clone()
    tied[V // 4] = 11.0
    tied[V // 2] = 11.0
    rows["tied_with_max_higher_index"] = (tied, V // 2, 1, V // 4)          # the maximum twice, the target at the higher index
    rows["tied_with_max_lower_index"] = (tied.clone(), V // 4, 0, V // 4)
    rows["id_first"] = (x.clone(), 0, None, None)
    rows["id_last"] = (x.clone(), V - 1, None, None)
    ext = x.clone()
    ext[3], ext[V - 2] = 65504.0, -65504.0
    rows["max_fp16_target_lowest"] = (ext, V - 2, V - 1, 3)                 # every other column lies above -65504
    rows["max_fp16_target_highest"] = (ext.clone(), 3, 0, 3)
    return rows


def fname(i):
    return "COCO_val2014_%012d.jpg" % i


def tool_fixture(root, O, S, write_packed, BertConfig):
    """The store, bert directory, checkpoint, image list and token file under `root`; the oracle module (parameter init only), vlp_amd.synthetic,
    vlp_amd.data.write_packed and BertConfig are passed in, so that importing this file needs none of them."""
    rng = np.random.RandomState(5)
    test_ids = [i for sp, i in LIST if sp == "test"]
    keys = [fname(i)[:-4] for i in reversed(test_ids)]
    feats = np.abs(rng.randn(5, NV, 2048)).astype(np.float16)
    cls = rng.rand(5, NV, 1601).astype(np.float32)
    cls /= cls.sum(-1, keepdims=True)
    xy = rng.rand(5, NV, 2, 2) * 400
    boxes = np.concatenate([xy.min(2), xy.max(2) + 1.0, np.zeros((5, NV, 1)), rng.rand(5, NV, 1)], axis=-1).astype(np.float32)
    store = os.path.join(root, "store")
    write_packed(store, keys, feats, cls, boxes)
    bert = os.path.join(root, "bert")
    os.makedirs(bert)
    with open(os.path.join(bert, "bert_config.json"), "w") as f:
        f.write(BertConfig(VOCAB, num_hidden_layers=2, type_vocab_size=2).to_json_string())
    special = {S.PAD_ID: "[PAD]", S.UNK_ID: "[UNK]", S.CLS_ID: "[CLS]", S.SEP_ID: "[SEP]", S.MASK_ID: "[MASK]"}
    tokens, n_ord = [], 0
    for i in range(VOCAB):
        if i in special:
            tokens.append(special[i])
        else:
            tokens.append(("##p%d" if n_ord % 3 == 2 else "w%d") % i)
            n_ord += 1
    with open(os.path.join(bert, "vocab.txt"), "w") as f:
        f.write("\n".join(tokens) + "\n")
    p = O.init_params(vocab_size=VOCAB, layers=2, tasks="img2txt", seed=27, std=0.1)
    sd = dict(p)
    sd["cls.predictions.decoder.weight"] = p["bert.embeddings.word_embeddings.weight"]
    ckpt = os.path.join(root, "model.3.bin")
    torch.save(sd, ckpt)
    src = os.path.join(root, "dataset.json")
    with open(src, "w") as f:
        json.dump({"images": [{"split": sp, "filename": fname(i), "filepath": "val2014", "imgid": n} for n, (sp, i) in enumerate(LIST)]}, f)
    examples = token_examples(test_ids, special)
    token_file = os.path.join(root, "tokens.json")
    with open(token_file, "w") as f:
        json.dump(examples, f)
    row_of = {k: r for r, k in enumerate(keys)}
    regions = {fname(i)[:-4]: (torch.from_numpy(feats[row_of[fname(i)[:-4]]]), torch.from_numpy(boxes[row_of[fname(i)[:-4]]]),
                               torch.from_numpy(cls[row_of[fname(i)[:-4]]].astype(np.float16))) for i in test_ids}
    return dict(root=root, store=store, bert=bert, ckpt=ckpt, src=src, tokens=tokens, test_ids=test_ids, regions=regions, token_file=token_file,
                examples=examples)


def token_examples(image_ids, special, seed=13):
    """[[store key, [token ids]]]: 2 or 3 captions per image (13 in all, so that batches of 2 and of 3 both end short), lengths 1..T - 1, one
    caption longer than T, and the first image's last caption placed at the end of the file, behind the other images'."""
    gen = torch.Generator().manual_seed(seed)
    ordinary = [i for i in range(VOCAB) if i not in special]
    per_image = [3, 2, 3, 2, 3]
    lengths = [4, 1, 7, T + 3, 5, 2, 9, T - 1, 3, 6, 8, 5, 4]
    out, held, k = [], None, 0
    for img, n in zip(image_ids, per_image):
        for j in range(n):
            pick = torch.randint(0, len(ordinary), (lengths[k],), generator=gen).tolist()
            ex = [fname(img)[:-4], [ordinary[q] for q in pick]]
            k += 1
            if img == image_ids[0] and j == n - 1:
                held = ex
            else:
                out.append(ex)
    return out + [held]
