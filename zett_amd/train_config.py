"""The four argument groups of the reference's entry point (train.py:81-163, zett/model/__init__.py:138-160) with its field names and
defaults, and the parse of a ``config.json`` into them.  A key no group knows is ignored, as the reference's ``parse_json_file`` ignores it."""
import json
import math
from dataclasses import dataclass
from typing import List, Optional


@dataclass
class TrainingArguments:
    output_dir: str
    init_from_params: str = None
    backbone_training: str = "no"  # or "full"
    resume_from_checkpoint: str = None
    resume_from_checkpoint_reset_steps: bool = False
    save_state: bool = True
    loss: str = "clm"
    mix_languages: bool = False
    use_adafactor: bool = False
    train_batch_size: int = 256
    eval_batch_size: int = 256
    learning_rate: float = 3e-4
    learning_rate_alpha: float = 0.1
    random_learning_rate: float = None
    max_grad_norm: float = None
    weight_decay: float = 0.0
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_epsilon: float = 1e-8
    steps: int = 100_000
    random_warmup_steps: int = 0
    identity_steps: int = 0
    warmup_steps: int = 10000
    logging_steps: int = 500
    save_steps: int = 10000
    eval_steps: int = 10000
    eval_at_step_zero: bool = False
    do_train: bool = True
    seed: int = 42
    gradient_accumulation_steps: int = 1
    debug: bool = False
    run_backbone_in_training_mode: bool = False
    learnable_bias: bool = False
    lexical_loss_weight: float = 0.0
    lexical_loss_kind: str = "mse"
    apply_lexical_loss_to_init: bool = False
    add_target_priors_to_bias: bool = True
    reinit_projectors: bool = False
    do_cost_analysis: bool = False


@dataclass
class ModelArguments:
    model_name_or_path: Optional[str] = None
    tokenizer_name: Optional[str] = None
    revision: Optional[str] = None
    config_name: Optional[str] = None
    dtype: Optional[str] = "float32"


@dataclass
class DataArguments:
    train_directory: str
    valid_directory: str
    langs: str
    use_passthrough_hypernet: bool = False
    do_sequence_packing: bool = True
    add_prefix_space: bool = True
    n_pools: int = 1
    language_sampling_alpha: float = 0.3
    block_size: int = 128
    extra_valid_tokenizer_names: List[str] = None
    extra_valid_files: List[str] = None
    extra_lang_codes: List[str] = None
    n_valid_subsample: int = None
    target_tokenizer_name: str = None
    pad_to_multiple_of: int = 128
    do_tokenizer_sampling: bool = True
    tokenizer_sample_reweigh_temperature: float = math.inf
    tokenizer_batch_size: int = 512
    tokenizer_sample_min: int = 16384
    tokenizer_sample_max: int = 32768
    tokenizer_sample_mean: float = 32768.0
    tokenizer_sample_std: float = 0.0
    tokenizer_noise_std: float = 0.0
    tokenizer_noise_mean: float = 0.0
    dataloader_num_workers: int = 64
    identity_n_subsample: int = None
    n_token_subsample: int = 8192
    sample_text_span: bool = True
    subsample_mode: str = "random"  # or "positives_only"


@dataclass
class HypernetArgs:
    hn_model_name_or_path: str = "out_xlmv_byte"
    hn_surface_maxlen: int = 16
    hn_n_layers: int = 3
    n_embd: int = 768
    hn_hidden_size: int = None
    hn_intermediate_size: int = None
    hn_rescale_embeddings: bool = False
    use_unigram_bias: bool = False
    hn_embed_target_priors: bool = False
    hn_add_inter_token_attention: bool = False
    hn_inter_token_attention_bias_by_priors: bool = False
    hn_inter_token_attention_bias_scaler: float = 1.0
    hn_n_inter_token_blocks: int = 16
    hn_language_adapter_bottleneck_dim: int = 0
    hn_embed_using_source_embeddings: bool = False
    hn_concat_last_hidden_state: bool = False
    hn_single_head: bool = False
    hn_predict_bias: bool = True
    hn_num_attention_heads: int = None
    hn_embed_lang_id: bool = False
    hn_model_type: str = "roberta"
    n_langs: int = None  # set by the entry point


GROUPS = (ModelArguments, DataArguments, TrainingArguments, HypernetArgs)


def parse_config(config):
    """``(model_args, data_args, training_args, hn_args)`` from a dict or the path of a JSON file, through ``HfArgumentParser``; keys that no
    group has are dropped"""
    from transformers import HfArgumentParser
    if not isinstance(config, dict):
        with open(config, encoding="utf-8") as f:
            config = json.load(f)
    return HfArgumentParser(GROUPS).parse_dict(config, allow_extra_keys=True)
