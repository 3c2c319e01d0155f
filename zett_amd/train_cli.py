"""``python scripts/train.py CONFIG.json``: the reference's entry point (train.py:194-870) for one process and one GPU, on
``HypernetTrainer``.  The config's keys are the reference's (zett_amd/train_config.py).  Metrics go to stdout and, one JSON object per
``log`` call, to ``output_dir/metrics.jsonl``.

Left out, each refused where it is asked for: training the backbone, ``apply_lexical_loss_to_init``, ``mix_languages``,
``use_passthrough_hypernet``, more than one language without ``lang,weight`` lines (the page counts that weigh languages are not
here), an ``init_from_params`` that is not a local directory, backbones other than causal language models and RoBERTa / XLM-R."""
import copy
import dataclasses
import json
import os
import sys
from typing import List, Optional, Tuple

import numpy as np
import torch

from .collate import MAX_CHARS_PER_TOKEN, DeviceCollator
from .config import ZettHypernetConfig
from .dataset import TrainDataset, ValidDataset, load_texts
from .train_config import parse_config
from .trainer import HypernetTrainer, device_loader, item_seed
from .training import init_hypernet_state

N_ANCHORS = 2048          # train.py:570
_LM_PRECISION = {"float32": "f32", "bfloat16": "bf16", "float16": "f16"}


def read_langs(spec: str) -> Tuple[List[str], np.ndarray]:
    """train.py:248-265: a space-separated string or a .txt file of language codes, one per line, optionally ``code,weight``"""
    probs = None
    if spec.endswith(".txt"):
        with open(spec, encoding="utf-8") as f:
            lines = [line.strip() for line in f if line.strip()]
        if "," in lines[0]:
            langs = [line.split(",")[0].strip() for line in lines]
            probs = np.array([float(line.split(",")[1].strip()) for line in lines])
            probs = probs / probs.sum()
        else:
            langs = lines
    else:
        langs = spec.split(" ")
    if len(langs) == 1:
        probs = np.array([1.0])
    elif probs is None:
        raise ValueError("more than one language needs weights: give langs as a .txt file of `lang,weight` lines")
    return langs, probs


def _pad_rows(x: torch.Tensor, multiple: int) -> torch.Tensor:
    extra = -x.shape[0] % multiple
    return x if extra == 0 else torch.cat([x, x.new_zeros((extra, x.shape[1]))])


def load_backbone(model_args, loss: str, pad_to_multiple_of: int, device):
    """-> (backbone(inputs_embeds, attention_mask) -> hidden, head or None, source_embeddings fp32 [V', E or 2E], the model's config).
    clm: any ``AutoModelForCausalLM`` whose ``base_model`` takes ``inputs_embeds``; mlm: RoBERTa / XLM-R, whose head transform becomes
    `head` and whose head bias is left out (train.py zeroes ``bias_path``)."""
    from transformers import AutoModelForCausalLM, AutoModelForMaskedLM
    dtype = getattr(torch, model_args.dtype)
    cls = {"clm": AutoModelForCausalLM, "mlm": AutoModelForMaskedLM}[loss]
    model = cls.from_pretrained(model_args.model_name_or_path, revision=model_args.revision, dtype=dtype).to(device).eval().requires_grad_(False)
    head = None
    if loss == "mlm":
        if model.config.model_type not in ("roberta", "xlm-roberta"):
            raise NotImplementedError(f"mlm backbone of type {model.config.model_type!r}: RoBERTa / XLM-R only")
        lm_head = model.lm_head
        head = lambda hidden: lm_head.layer_norm(torch.nn.functional.gelu(lm_head.dense(hidden)))          # noqa: E731
    base = model.base_model
    if base is model:
        raise NotImplementedError(f"{type(model).__name__} has no base model to feed inputs_embeds to")
    backbone = lambda inputs_embeds, attention_mask: base(inputs_embeds=inputs_embeds, attention_mask=attention_mask).last_hidden_state          # noqa: E731
    source = _pad_rows(model.get_input_embeddings().weight.detach().float(), pad_to_multiple_of)
    if not model.config.tie_word_embeddings:
        source = torch.cat([source, _pad_rows(model.get_output_embeddings().weight.detach().float(), pad_to_multiple_of)], dim=1)
    return backbone, head, source.contiguous(), model.config


def load_pretrained_state(path: str):
    """``init_from_params``: a local directory with ``flax_model.msgpack`` or with the layout ``ZettHypernet.from_pretrained`` reads"""
    if not os.path.isdir(path):
        raise NotImplementedError(f"init_from_params={path!r} is not a local directory (nothing is downloaded)")
    msgpack = os.path.join(path, "flax_model.msgpack")
    if os.path.exists(msgpack):
        from .flax_io import load_flax_checkpoint
        return {k: torch.from_numpy(v) for k, v in load_flax_checkpoint(msgpack).items()}
    from .hypernet import ZettHypernet
    return dict(ZettHypernet.from_pretrained(path).state_dict())


def _spans(texts, block_size: int, sample: bool, rng):
    n = MAX_CHARS_PER_TOKEN * block_size
    out = []
    for text in texts:
        start = int(rng.integers(0, max(len(text) - n, 0) + 1)) if sample else 0
        out.append(text[start:start + n])
    return out


def warm_samplers(initial_texts, data_args, batch_size: int, rng, device):
    """collator.py:120-151: per language ``n_pools`` samplers, each fed the initial texts in chunks of `batch_size`"""
    from .tokenizer_sampling import DeviceTokenizerSampler
    samplers = {}
    for lang, texts in initial_texts.items():
        texts = _spans(texts, data_args.block_size, data_args.sample_text_span, rng)
        samplers[lang] = []
        for _ in range(data_args.n_pools):
            sampler = DeviceTokenizerSampler(device=device)
            for start in range(0, len(texts), batch_size):
                sampler.sample_tokenizer({text: 1 for text in texts[start:start + batch_size]}, 30_000, 16, 4, 0.0, False)
            samplers[lang].append(sampler)
    return samplers


def main(argv: Optional[List[str]] = None) -> None:
    from transformers import AutoTokenizer

    from .byte_level import convert_to_byte_level
    from .hypernet import ZettHypernet
    from .surface_forms import get_surface_form_matrix
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1 or not argv[0].endswith(".json"):
        raise SystemExit("usage: train.py CONFIG.json")
    model_args, data_args, training_args, hn_args = parse_config(os.path.abspath(argv[0]))
    name = os.path.splitext(os.path.basename(argv[0]))[0]
    if data_args.use_passthrough_hypernet:
        raise NotImplementedError("use_passthrough_hypernet")
    device = torch.device("cuda", 0)
    os.makedirs(training_args.output_dir, exist_ok=True)
    data_args.hn_surface_maxlen = hn_args.hn_surface_maxlen
    langs, train_probs = read_langs(data_args.langs)
    data_args.langs = langs
    hn_args.n_langs = len(langs)
    seed = int(training_args.seed)
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)

    reference = AutoTokenizer.from_pretrained(model_args.tokenizer_name or model_args.model_name_or_path)
    if reference.pad_token is None:
        reference.pad_token = reference.eos_token
    backbone, head, source_embeddings, model_config = load_backbone(model_args, training_args.loss, data_args.pad_to_multiple_of, device)
    hn_tokenizer, hn_n_extra_tokens = None, None
    if hn_args.hn_embed_using_source_embeddings:
        hn_tokenizer, hn_n_extra_tokens = convert_to_byte_level(copy.deepcopy(reference))
    elif hn_args.hn_model_name_or_path is not None:
        hn_tokenizer, hn_n_extra_tokens = convert_to_byte_level(AutoTokenizer.from_pretrained(hn_args.hn_model_name_or_path))
    config = ZettHypernetConfig(**dataclasses.asdict(hn_args), pad_token_id=reference.pad_token_id, original_vocab_size=model_config.vocab_size,
                                vocab_size=model_config.vocab_size + int(hn_n_extra_tokens or 0), separate_out_embeddings=not model_config.tie_word_embeddings,
                                hn_n_extra_tokens=hn_n_extra_tokens, name=name, langs=langs)

    # data (train.py:378-556)
    loss, sampling = training_args.loss, bool(data_args.do_tokenizer_sampling)
    # (packed texts hold the eos string between their rows: the collator's encoders split added tokens out of a text as the library does)
    train_datasets = [TrainDataset([lang], data_args.train_directory, np.array([1.0]), training_args.train_batch_size, data_args.block_size,
                                   do_sequence_packing=data_args.do_sequence_packing, eos_token=reference.eos_token) for lang in langs]
    target = None if sampling else AutoTokenizer.from_pretrained(data_args.target_tokenizer_name)

    def collator(args, *, samplers=None, tokenizer=None, **kw):
        return DeviceCollator(reference, hn_tokenizer, args, loss=loss, tokenizer=tokenizer, samplers=samplers, device=device, **kw)

    if sampling:
        initial = {lang: dset.get_texts(data_args.tokenizer_batch_size) for lang, dset in zip(langs, train_datasets)}
        train_collators = [collator(data_args, samplers=warm_samplers({lang: initial[lang]}, data_args, training_args.train_batch_size, rng, device)) for lang in langs]
        valid_collator = collator(data_args, samplers=warm_samplers(initial, data_args, training_args.train_batch_size, rng, device), is_validation=True)
    else:
        train_collators = [collator(data_args, tokenizer=target) for _ in langs]
        valid_collator = collator(data_args, tokenizer=target, is_validation=True)
    train_loaders = [device_loader(dset, c, seed=item_seed(seed, 1 + j)) for j, (dset, c) in enumerate(zip(train_datasets, train_collators))]
    valid_dataset = ValidDataset(langs, data_args.valid_directory, data_args.n_valid_subsample, training_args.eval_batch_size)
    eval_sets = {}
    for i, tokenizer_name in enumerate(data_args.extra_valid_tokenizer_names or []):
        extra_args = copy.deepcopy(data_args)
        extra_args.do_tokenizer_sampling, extra_args.n_token_subsample, extra_args.sample_text_span = False, None, False
        path = data_args.extra_valid_files[i]
        texts = load_texts(os.path.dirname(path), os.path.splitext(os.path.basename(path))[0], "validation", data_args.n_valid_subsample)
        b = training_args.eval_batch_size
        items = [{"texts": list(texts[k * b:(k + 1) * b]), "lang_code": data_args.extra_lang_codes[i]} for k in range(len(texts) // b)]          # drop_last
        extra = collator(extra_args, tokenizer=AutoTokenizer.from_pretrained(tokenizer_name), is_validation=True, lang_code=data_args.extra_lang_codes[i])
        eval_sets[(tokenizer_name + "_" + os.path.splitext(path)[0]).replace("/", "_")] = device_loader(items, extra, seed=item_seed(seed, 1000 + i))
    eval_sets["main"] = device_loader(valid_dataset, valid_collator, seed=item_seed(seed, 999))
    identity_loader = None
    if training_args.identity_steps > 0:
        identity_args = copy.deepcopy(data_args)
        identity_args.do_tokenizer_sampling = False
        if hn_args.hn_embed_using_source_embeddings:
            identity_args.hn_surface_maxlen = 1
        if data_args.identity_n_subsample is not None:
            identity_args.n_token_subsample = data_args.identity_n_subsample
        identity_loader = device_loader(None, collator(identity_args, tokenizer=copy.deepcopy(reference), lang_code=langs[0]), seed=item_seed(seed, 0),
                                        for_identity_step=True, length=training_args.identity_steps)

    # the hypernetwork (train.py:568-576, 689-725)
    hypernet = ZettHypernet(config)
    pretrained = load_pretrained_state(training_args.init_from_params) if training_args.init_from_params is not None else None
    hypernet = hypernet.to(device).requires_grad_(True).train()
    anchors = get_surface_form_matrix(convert_to_byte_level(copy.deepcopy(reference))[0], hn_args.hn_surface_maxlen, hn_tokenizer, device=device)[0][:N_ANCHORS]
    init_hypernet_state(hypernet, source_embeddings, torch.from_numpy(np.ascontiguousarray(anchors)).to(device), pretrained_state=pretrained,
                        reinit_projectors=training_args.reinit_projectors)
    if model_args.dtype in ("bfloat16", "float16"):
        hypernet.train_precision = _LM_PRECISION[model_args.dtype]
    trainer = HypernetTrainer(hypernet, backbone, source_embeddings, training_args, hn_pad_token_id=None if hn_tokenizer is None else hn_tokenizer.pad_token_id, head=head,
                              lm_precision=_LM_PRECISION[model_args.dtype], embed_dtype=getattr(torch, model_args.dtype), langs=langs, hn_tokenizer=hn_tokenizer)
    if training_args.resume_from_checkpoint is not None:
        trainer.resume(training_args.resume_from_checkpoint)

    metrics_file = open(os.path.join(training_args.output_dir, "metrics.jsonl"), "a", encoding="utf-8")

    def log(metrics, step):
        print(metrics, flush=True)
        metrics_file.write(json.dumps(dict(metrics, step=step)) + "\n")
        metrics_file.flush()

    try:
        if training_args.do_train:
            trainer.fit(train_loaders, train_probs, identity_loader=identity_loader, eval_sets=eval_sets, log=log)
        else:
            log(trainer.evaluate(eval_sets), 0)
    finally:
        metrics_file.close()


if __name__ == "__main__":
    main()
