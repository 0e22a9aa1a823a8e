"""Configuration for the MI355X-native HeteroFL engine.

The reference keeps a global mutable ``cfg`` dict loaded from YAML at import
time (reference: src/config.py:1-6) and mirrors every key into argparse flags
(src/train_classifier_fed.py:20-30).  We keep the same *surface* — a module
level ``cfg`` dict and the same key names — but the defaults live in code, the
YAML file is optional, and nothing happens at import time beyond building the
default dict.
"""
import copy
import os

import yaml

_DEFAULT = {
    # control block — field order defines the control_name grammar
    # (reference: src/config.yml:3-12)
    'control': {
        'fed': '1',
        'num_users': '100',
        'frac': '0.1',
        'data_split_mode': 'iid',
        'model_split_mode': 'fix',
        'model_mode': 'a1',
        'norm': 'bn',
        'scale': '1',
        'mask': '1',
    },
    # data
    'data_name': 'CIFAR10',
    'subset': 'label',
    'batch_size': {'train': 128, 'test': 128},
    'shuffle': {'train': True, 'test': False},
    'num_workers': 0,
    'model_name': 'resnet18',
    'metric_name': {'train': ['Loss', 'Accuracy'], 'test': ['Loss', 'Accuracy']},
    # optimizer
    'optimizer_name': 'Adam',
    'lr': 3.0e-4,
    'momentum': 0.9,
    'weight_decay': 5.0e-4,
    # scheduler
    'scheduler_name': 'None',
    'step_size': 1,
    'milestones': [100, 150],
    'patience': 10,
    'threshold': 1.0e-3,
    'factor': 0.5,
    'min_lr': 1.0e-4,
    # experiment
    'init_seed': 0,
    'num_experiments': 1,
    'num_epochs': 200,
    'log_interval': 0.25,
    'device': 'cuda',
    'world_size': 1,
    'resume_mode': 0,
    # other
    'save_format': 'pdf',
    # engine selection (new): 'sequential' replicates the reference's one
    # client at a time loop; 'batched' trains all same-rate active clients in
    # one grouped model (MI355X-native fast path).
    'engine': 'batched',
    # Compute dtype for local training on GPU ('float32' or 'bfloat16').
    'compute_dtype': 'float32',
    # Use hand-written HIP kernels when the extension is available.
    'native_ops': True,
    # Capture the local-training step in a hipGraph on GPU.
    'hip_graphs': True,
    # Sub-model extraction: 'static' hands every client the first channels
    # of each layer; 'roll' moves the extraction window by roll_step
    # positions per round so all global channels are trained evenly.
    'submodel': 'static',
    'roll_step': 1,
}


def default_config():
    return copy.deepcopy(_DEFAULT)


def load_config(path=None):
    """Return the default config, updated from a YAML file if one is given
    (or if ``config.yml`` exists next to the caller's cwd)."""
    out = default_config()
    if path is None and os.path.exists('config.yml'):
        path = 'config.yml'
    if path is not None and os.path.exists(path):
        with open(path) as f:
            user = yaml.safe_load(f) or {}
        out.update(user)
    return out


# Module-level cfg for reference-API parity.  Entry scripts mutate this in
# place (via cfg.update(...)) before calling process_control().
cfg = load_config()
