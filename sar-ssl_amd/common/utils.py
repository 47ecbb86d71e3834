"""Seeding, parameter counting and the cosine learning-rate schedule (code/common/utils.py:39-56, 59-72, 108-139)."""
import json
import os
import random

import numpy as np
import torch

from ..runtime import RT


def set_seed(seed):
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    RT.manual_seed(seed)


set_random_seed = set_seed


def get_nparams(model, param_key_list=[]):
    nparam_sum = 0.0
    nparam = {k: 0 for k in param_key_list}
    for key, value in model.named_parameters():
        nparam_sum += value.numel() / 1000000
        for k in param_key_list:
            if k in key:
                nparam[k] += value.numel() / 1000000
    return nparam, nparam_sum


def create_learning_rate_schedule(total_steps, base, decay_type, warmup_steps, linear_end=1e-5):
    def step_fn(step):
        lr = base
        if total_steps > warmup_steps:
            progress = np.clip((step - warmup_steps) / float(total_steps - warmup_steps), 0.0, 1.0)
        else:       # nothing behind the warm-up (`--nepoch 1` with its one warm-up epoch): no decay yet, where the reference divides by zero
            progress = 0.0 if step <= warmup_steps else 1.0
        if decay_type == "linear":
            lr = linear_end + (lr - linear_end) * (1.0 - progress)
        elif decay_type == "cosine":
            lr = lr * 0.5 * (1.0 + np.cos(np.pi * progress))
        else:
            raise ValueError(f"Unknown lr type {decay_type}")
        if warmup_steps:
            lr = lr * np.minimum(1.0, step / warmup_steps)
        return np.asarray(lr, dtype=np.float32)
    return step_fn


def cross_validation_datadir(data_dir, sort=False):
    """Leave-one-room-out splits of a directory of rooms (code/common/utils.py:249-277): one trial per room in ``os.listdir`` order with
    that room as the test set, one of the others drawn with ``random.sample`` as the validation set, the rest for training.
    sort=True: rooms in sorted order instead of the file system's.  -> [{'train': [dirs], 'val': [dir], 'test': [dir]}]."""
    room_names = sorted(os.listdir(data_dir)) if sort else os.listdir(data_dir)
    dirs = []
    for test_room_name in room_names:
        trainval = [r for r in room_names if r != test_room_name]
        val_room_name = random.sample(trainval, 1)[0]
        dirs += [{"train": [data_dir + "/" + r for r in trainval if r != val_room_name], "val": [data_dir + "/" + val_room_name],
                  "test": [data_dir + "/" + test_room_name]}]
    return dirs


def vis_TSNE(data, label):
    """t-SNE scatter of ``data`` (nins, dim) coloured by ``label`` (code/common/utils.py:280-291) -> (pyplot, {'data': (nins, 2), 'label'}).
    sklearn and matplotlib are imported here, not with the package: a caller without them catches the ImportError.  sklearn refuses
    a perplexity (default 30) >= nins, so for nins <= 30 ``max(1, (nins - 1) // 3)`` is passed; the reference never meets so few points."""
    from sklearn.manifold import TSNE
    import matplotlib.pyplot as plt
    plt.switch_backend("agg")
    n = len(data)
    kwargs = {"perplexity": max(1, (n - 1) // 3)} if n <= 30 else {}
    data_vis = TSNE(n_components=2, learning_rate=100, **kwargs).fit_transform(data)
    plt.figure(figsize=(4, 3.2))
    p = plt.scatter(data_vis[:, 0], data_vis[:, 1], c=label, s=15, marker="o", cmap="plasma")
    plt.colorbar(p)
    return plt, {"data": data_vis, "label": label}


def save_config_to_file(config, file_path):
    with open(file_path, "w") as f:
        json.dump(config, f, indent=4, default=str)
