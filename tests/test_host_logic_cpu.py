"""CPU: host-side logic of the product package that needs no kernels — config objects, module surface / state_dict keys,
LR schedule, synthetic batch schema, reducer bucket planning."""
import os

import torch

from oracle import sa_m4c_oracle as O
from tests import oracle_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_from_dict_copies_every_key():
    import sam_textvqa_amd.modules as M
    c = M.BertConfig.from_dict(dict(hidden_size=96, layer_type_list=["n", "s"], mix_list=["none", "share3"], foo=1))
    assert c.hidden_size == 96 and c.layer_type_list == ["n", "s"] and c.foo == 1 and c.layer_norm_eps == 1e-12
    assert c.attention_probs_dropout_prob == 0.1 and c.intermediate_size == 3072


def test_module_surface_and_state_dict_keys_equal_oracle():
    import sam_textvqa_amd.modules as M
    mcfg, tcfg = OC.sam4c_configs("sam4c_small_c3")
    kw = dict(mcfg.__dict__, hidden_size=768, intermediate_size=128, ptr_query_size=768)
    model = M.SAM4C(M.BertConfig.from_dict(kw), M.BertConfig.from_dict(tcfg.__dict__), num_answers=30, bos_idx=1)
    ref = O.SAM4C(O.BertConfig.from_dict(kw), O.BertConfig.from_dict(tcfg.__dict__), num_answers=30)
    assert list(model.state_dict()) == list(ref.state_dict())
    for k, v in ref.state_dict().items():
        assert model.state_dict()[k].shape == v.shape, k
    model.load_state_dict(ref.state_dict())                       # a reference-layout checkpoint is a drop-in
    groups = model.get_optimizer_parameters(1e-4)
    assert [len(g["params"]) for g in groups] == [len(g["params"]) for g in ref.get_optimizer_parameters(1e-4)]
    assert "lr" not in groups[0] and groups[1]["lr"] == 1e-4
    for name in ("SpatialBertSelfAttention", "SpatialBertAttention", "SpatialBertLayer", "BertSpatialEncoder", "MMT", "OcrPtrNet",
                 "PrevPredEmbeddings", "TextBert", "BertLayerNorm", "SAM4C"):
        assert hasattr(M, name)


def test_unsupported_options_raise():
    import pytest
    import sam_textvqa_amd.modules as M
    base = dict(hidden_size=768, num_spatial_relations=12, max_seq_length=4, num_decoding_steps=2, attention_mask_quadrants=[1, 2])
    # use_bias (sa_m4c.py:439-443) is built since round 6: the head-bias row exists under the reference's state_dict key, and is absent by default
    att = M.SpatialBertSelfAttention(M.BertConfig.from_dict(dict(base, use_bias=True)))
    assert tuple(att.state_dict()["biases.weight"].shape) == (1, 768)
    assert "biases.weight" not in M.SpatialBertSelfAttention(M.BertConfig.from_dict(base)).state_dict()
    with pytest.raises(NotImplementedError):          # head_mask: one factor per head, nothing finer
        M._head_scale(torch.ones(2, 12, 4, 4), 12, "cpu")
    assert M._head_scale(torch.full((1, 12, 1, 1), 0.5), 12, "cpu").shape == (12,) and M._head_scale(None, 12, "cpu") is None
    with pytest.raises(ValueError):
        M.SpatialBertSelfAttention(M.BertConfig.from_dict(dict(base, hidden_size=100)))
    with pytest.raises(NotImplementedError):
        M.BertIntermediate(M.BertConfig.from_dict(dict(base, hidden_act="relu")))


def test_lr_schedule_matches_oracle():
    from sam_textvqa_amd.trainer import lr_lambda
    for it in (0, 1, 500, 1000, 1001, 13999, 14000, 18999, 19000, 50000):
        assert lr_lambda(it) == O.lr_lambda(it)
    assert lr_lambda(10, warmup_iters=20, warmup_factor=0.5) == 0.75


def test_synthetic_batch_schema_cpu():
    from sam_textvqa_amd.synthetic import clone_batch, make_batch
    bd = make_batch(3, vocab=100, device="cpu", seed=7)
    shapes = {"pad_obj_features": (3, 100, 2048), "pad_obj_bboxes": (3, 100, 5), "pad_ocr_bboxes": (3, 50, 5), "pad_obj_mask": (3, 100),
              "pad_ocr_mask": (3, 50), "pad_ocr_features": (3, 50, 2048), "ocr_fasttext": (3, 50, 300), "ocr_phoc": (3, 50, 604),
              "question_indices": (3, 20), "question_mask": (3, 20), "train_prev_inds": (3, 12), "targets": (3, 12, 150), "train_loss_mask": (3, 12)}
    for k, s in shapes.items():
        assert tuple(bd[k].shape) == s, k
    adj = bd["spatial_adj_matrices"]["3"]
    assert adj.dtype == torch.int8 and tuple(adj.shape) == (3, 150, 150, 12)
    assert bd["pad_obj_mask"].dtype == torch.long and bd["train_prev_inds"].dtype == torch.long and (bd["train_prev_inds"][:, 0] == 1).all()
    # padded OCR boxes are all-zero and carry no relations; valid diagonal = relation 12
    n_ocr = bd["pad_ocr_mask"].sum(1)
    for b in range(3):
        assert (adj[b, 100 + n_ocr[b]:, :, :] == 0).all() and (adj[b, :, 100 + n_ocr[b]:, :] == 0).all()
        assert (adj[b, torch.arange(100), torch.arange(100), 11] == 1).all()
    # the oracle runs on it (same schema as the reference's batch_dict)
    c2 = clone_batch(bd)
    assert c2 is not bd and c2["targets"] is bd["targets"]
    dens = adj[:, :100, :100, 3:11].float().mean().item()
    assert 0.2 < dens < 0.45, dens           # c=3: ~1/3 of valid pairs on each sector head


def test_reducer_bucket_plan_and_region_order():
    from sam_textvqa_amd.parallel import GradReducer
    g = torch.zeros(1000)
    red = GradReducer(g, bucket_bytes=4 * 256)
    assert red.buckets == [(744, 1000), (488, 744), (232, 488), (0, 232)]
    ids = red.register_regions([(100, 300), (300, 600), (600, 1000)])      # layers in address order
    assert ids == [2, 1, 0]
    # every region boundary is a bucket boundary (round 6; rounds 2-5 cut only at the low end of the regions): no bucket waits for a region it does not belong to
    assert red.buckets == [(744, 1000), (600, 744), (344, 600), (300, 344), (100, 300), (0, 100)]
    red.mark_done(ids[0])                      # lowest layer finishing first releases nothing
    assert red.next_bucket == 0
    red.mark_done(ids[2]); assert red.next_bucket == 2          # [600,1000) complete: both of its buckets
    red.mark_done(ids[1]); assert red.next_bucket == 5          # everything >= 100 final -> every bucket of the region range
    red.finish(); assert red.next_bucket == 6
    red2 = GradReducer(torch.zeros(1000), bucket_bytes=4 * 256, dense_lo=40)     # row-sparse table in [0, 40): outside every bucket
    red2.register_regions([(500, 1000)])
    assert red2.buckets == [(744, 1000), (500, 744), (244, 500), (40, 244)]


def test_reducer_with_the_sparse_table_in_the_middle():
    """three optimizer groups (text_bert_init_from_bert_base): the word-embedding table sits between the default group and the rest of
    TextBert; it is in no dense bucket, and regions may continue below it"""
    from sam_textvqa_amd.parallel import GradReducer
    red = GradReducer(torch.zeros(1000), bucket_bytes=4 * 200, sparse_range=(300, 400))
    assert red.buckets == [(800, 1000), (600, 800), (400, 600), (100, 300), (0, 100)] and red.dense_lo == 0
    ids = red.register_regions([(250, 300), (400, 700), (700, 1000)])      # a region below the table, two above
    assert ids == [2, 1, 0]
    assert red.buckets == [(800, 1000), (700, 800), (500, 700), (400, 500), (250, 300), (50, 250), (0, 50)]
    red.set_barrier(("a", "b"), [ids[0], ids[2]])       # one barrier may finalise several (non-adjacent) regions
    red.barrier_hit("a"); assert red.next_bucket == 0
    red.barrier_hit("b"); assert red.next_bucket == 2     # [700,1000) final; [250,300) is too but must wait for everything above it
    red.mark_done(ids[1]); assert red.next_bucket == 5    # ... and leaves as soon as the middle region is done
    red.finish(); assert red.next_bucket == 7
    import pytest
    with pytest.raises(ValueError):
        GradReducer(torch.zeros(1000), sparse_range=(300, 400)).register_regions([(200, 290), (400, 1000)])    # a real gap


def test_three_optimizer_groups_when_text_bert_starts_from_bert_base(tmp_path):
    """sa_m4c.py:74-85,349-371: [default lr | text_bert @ lr_scale_text_bert | mmt @ lr_scale_mmt], weights from a local bert-base file"""
    import sam_textvqa_amd.modules as M
    mcfg, tcfg = OC.sam4c_configs("sam4c_small_c3")
    kw = dict(mcfg.__dict__, hidden_size=768, intermediate_size=128, ptr_query_size=768)
    tkw = dict(tcfg.__dict__, text_bert_init_from_bert_base=True, lr_scale_text_bert=0.1)
    plain = M.SAM4C(M.BertConfig.from_dict(kw), M.BertConfig.from_dict(tcfg.__dict__), num_answers=30, bos_idx=1)
    # a stand-in "bert-base-uncased" file in the usual key layout (bert. prefix, 12 layers, old gamma/beta LayerNorm names)
    fake = {}
    for k, v in plain.text_bert.state_dict().items():
        fake["bert." + k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta")] = torch.randn_like(v)
    fake["bert.encoder.layer.11.output.dense.bias"] = torch.zeros(768)
    fake["cls.predictions.bias"] = torch.zeros(5)
    path = str(tmp_path / "pytorch_model.bin")
    torch.save(fake, path)
    model = M.SAM4C(M.BertConfig.from_dict(kw), M.BertConfig.from_dict(dict(tkw, text_bert_pretrained_path=str(tmp_path))), num_answers=30, bos_idx=1)
    assert torch.equal(model.text_bert.embeddings.LayerNorm.weight, fake["bert.embeddings.LayerNorm.gamma"])
    assert torch.equal(model.text_bert.encoder.layer[0].attention.self.query.weight, fake["bert.encoder.layer.0.attention.self.query.weight"])
    groups = model.get_optimizer_parameters(1e-4)
    n_tb, n_mmt = len(list(model.text_bert.parameters())), len(list(model.mmt.parameters()))
    assert [len(g["params"]) for g in groups] == [len(list(model.parameters())) - n_tb - n_mmt, n_tb, n_mmt]
    assert "lr" not in groups[0] and abs(groups[1]["lr"] - 1e-5) < 1e-12 and groups[2]["lr"] == 1e-4
    assert list(model.state_dict()) == list(plain.state_dict())          # same checkpoint layout either way
    # without a local file the flag is still accepted (the weights then come from a checkpoint)
    m2 = M.SAM4C(M.BertConfig.from_dict(kw), M.BertConfig.from_dict(tkw), num_answers=30, bos_idx=1)
    assert len(m2.get_optimizer_parameters(1e-4)) == 3


def test_shipped_reference_configs_build_the_model_unchanged():
    """every shipped reference config (configs/*.yml; their model-facing keys stored in tests/golden/reference_configs.json by make_golden.py)
    -> BertConfig.from_dict -> SAM4C(mmt_config, text_bert_config) exactly as train.py:92-94 does"""
    import json, os
    import pytest
    import sam_textvqa_amd.modules as M
    from sam_textvqa_amd.registry import registry
    registry.answer_vocab, registry.BOS_IDX = list(range(5000)), 1         # what the dataset code puts there (sa_m4c.py:169,291)
    configs = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")))
    assert len(configs) == 4
    for f, cfg in sorted(configs.items()):
        mmt_config, text_bert_config = M.BertConfig.from_dict(cfg["SA-M4C"]), M.BertConfig.from_dict(cfg["TextBERT"])
        model = M.SAM4C(mmt_config, text_bert_config)
        groups = model.get_optimizer_parameters(cfg["lr"])
        assert [len(g["params"]) for g in groups] == [22, 53, 104], os.path.basename(f)        # SURVEY.md App. B probe: 75 + 104 without the flag
        assert "lr" not in groups[0] and abs(groups[1]["lr"] - 0.1 * cfg["lr"]) < 1e-12 and groups[2]["lr"] == cfg["lr"]
        assert sum(p.numel() for p in model.parameters()) == 96_633_224, os.path.basename(f)          # 96.63 M
        enc = model.mmt.encoder
        assert (len(enc.normal_layers), len(enc.spatial_layers)) == (2, 4) and enc.mix_list == cfg["SA-M4C"]["mix_list"]
        # the shipped c5 file asks the MODEL for share5 heads while its top-level (dataset) mix_list says share3: the reference dies with a bare
        # KeyError('5') at sa_m4c.py:747; this build names the mismatch
        if enc.mix_list[-1] != cfg["mix_list"][-1]:
            bd = {"spatial_adj_matrices": {"3": None, "1": None}}
            with pytest.raises(KeyError, match="mix_list"):
                enc._adjacency_for(bd, enc.mix_list[-1])


def test_bench_issues_no_collective_after_the_ranks_part_ways():
    """bench.py sent ranks != 0 into the closing barrier and let rank 0 run four more data-parallel steps alone -- mismatched collectives,
    no JSON line at N > 1.  Everything that enqueues a collective (a trainer step under a reducer, an all-reduce, the exposed-communication read-out) must
    sit BEFORE the `if rank != 0:` return; behind it rank 0 may only compute locally, print, and meet the others in ONE closing barrier."""
    import ast
    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    split = None
    for i, node in enumerate(main.body):
        if isinstance(node, ast.If) and isinstance(node.test, ast.Compare) and getattr(node.test.left, "id", None) == "rank" \
                and isinstance(node.test.ops[0], ast.NotEq) and any(isinstance(x, ast.Return) for x in node.body):
            split = i
    assert split is not None, "bench.py no longer has the rank != 0 early return this test anchors on"
    tail = ast.Module(body=main.body[split + 1:], type_ignores=[])
    barriers = 0
    for node in ast.walk(tail):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute):
            name = node.func.attr
            owner = ast.unparse(node.func.value)
            if name == "barrier":
                barriers += 1
                continue
            assert not (name == "step" and owner == "trainer"), "trainer.step() behind the rank split (line %d)" % node.lineno
            assert name not in ("all_reduce", "all_gather", "all_gather_into_tensor", "broadcast", "reduce_scalar", "all_to_all_single"), \
                "collective %s behind the rank split (line %d)" % (name, node.lineno)
            assert not (name == "exposed_comm_ms"), "exposed_comm_ms() behind the rank split (line %d): it closes a leg every rank must run" % node.lineno
    assert barriers == 1
    # the rank != 0 branch itself: one barrier (the partner of rank 0's closing one), destroy, return
    node = main.body[split]
    calls = [n.func.attr for n in ast.walk(node) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)]
    assert calls == ["barrier", "destroy_process_group"], calls
