#!/usr/bin/env python3
"""Representation-change experiment (reference misc_scripts/rc_vision.py:34-99,150-165): adapt a clone of the model to each
task and collect, per layer, the representation of the adaptation data before and after adaptation.  The similarity measures
(CCA / CKA, ``utils/cca.py``, ``utils/cka.py``) run on the returned arrays, or on the device in ``run_rep_cca`` / ``run_rep_cka``."""
import numpy as np
import torch

from ..core_functions import accuracy, prepare_batch
from ..utils.cca import cca
from ..utils.cka import cka

default_params = {"adapt_steps": 1, "inner_lr": 0.1, "n_tasks": 5, "layers": [0, 1, 2, 3, 4]}


def get_rep_from_batch(model, batch, layer=4):
    """reference rc_vision.py:150-165: [features, batch] matrix of the layer's representation (layer -1: the logits)."""
    if layer == -1:
        return model(batch).cpu().detach().numpy()
    rep = model.get_rep_i(batch, layer).cpu().detach().numpy()
    b, c, h, w = rep.shape
    return rep.reshape((c * h * w, b))


def run_rep_exp(model, loss, tasks, device, ways, shots, rep_params=default_params):
    """Returns (acc_results [n_tasks, 2] = (adapted, initial) accuracy on the evaluation half, reps) with
    reps[layer] = list over tasks of (adapted_rep, init_rep) as produced by get_rep_from_batch."""
    init_model = model.clone()
    adapt_model = model.clone()                     # adapted cumulatively over the tasks, like the reference (:48-70)
    acc = np.zeros((rep_params['n_tasks'], 2))
    reps = {int(layer): [] for layer in rep_params['layers']}
    for t in range(rep_params['n_tasks']):
        adapt_d, adapt_l, eval_d, eval_l = prepare_batch(tasks.sample(), shots, ways, device)
        for _ in range(rep_params['adapt_steps']):
            train_error = loss(adapt_model(adapt_d), adapt_l)
            train_error = train_error / len(adapt_d)                     # reference :69
            adapt_model.adapt(train_error)
            acc[t, 0] = accuracy(adapt_model(eval_d), eval_l).item()
            acc[t, 1] = accuracy(init_model(eval_d), eval_l).item()
        for layer in reps:
            reps[layer].append((get_rep_from_batch(adapt_model, adapt_d, layer), get_rep_from_batch(init_model, adapt_d, layer)))
    return acc, reps


def _device_rep(model, batch, layer):
    """get_rep_from_batch's [c*h*w, b] matrix (a reshape of the contiguous [b, c, h, w] rep, not a transpose), kept on the device."""
    if layer == -1:
        return model(batch).detach()
    rep = model.get_rep_i(batch, layer).detach()
    b, c, h, w = rep.shape
    return rep.reshape((c * h * w, b))


def run_rep_cka(model, loss, tasks, device, ways, shots, rep_params=default_params, sigma=None):
    """run_rep_exp's loop with the CKA the reference leaves commented out (rc_vision.py:89-91): per layer, linear and RBF-kernel
    CKA (utils/cka.py) between the adapted and the initial representation of each task's adaptation data, as ONE batched GPU
    call per layer over all tasks.  Returns (acc [n_tasks, 2], {'linear': {layer: [n_tasks floats]}, 'kernel': {...}})."""
    init_model = model.clone()
    adapt_model = model.clone()
    acc = np.zeros((rep_params['n_tasks'], 2))
    layers = [int(layer) for layer in rep_params['layers']]
    reps = {layer: ([], []) for layer in layers}
    for t in range(rep_params['n_tasks']):
        adapt_d, adapt_l, eval_d, eval_l = prepare_batch(tasks.sample(), shots, ways, device)
        for _ in range(rep_params['adapt_steps']):
            train_error = loss(adapt_model(adapt_d), adapt_l)
            train_error = train_error / len(adapt_d)
            adapt_model.adapt(train_error)
            acc[t, 0] = accuracy(adapt_model(eval_d), eval_l).item()
            acc[t, 1] = accuracy(init_model(eval_d), eval_l).item()
        for layer in layers:
            reps[layer][0].append(_device_rep(adapt_model, adapt_d, layer))
            reps[layer][1].append(_device_rep(init_model, adapt_d, layer))
    results = {'linear': {}, 'kernel': {}}
    for layer in layers:
        r = cka(torch.stack(reps[layer][0]), torch.stack(reps[layer][1]), sigma)
        results['linear'][layer] = r.linear.cpu().tolist()
        results['kernel'][layer] = r.kernel.cpu().tolist()
    return acc, results


def run_rep_cca(model, loss, tasks, device, ways, shots, rep_params=default_params, epsilon=1e-10):
    """run_rep_exp's loop with the measure the reference runs (rc_vision.py:84-88): per layer, the mean canonical correlation
    ``get_cca_similarity(adapted_rep.T, init_rep.T, epsilon=1e-10)[1]`` (utils/cca.py) between the adapted and the initial
    representation of each task's adaptation data, as ONE batched GPU call per layer over all tasks.  Returns
    (acc [n_tasks, 2], {layer: [n_tasks floats]}); the dict is what the reference dumps as cca_results.json (:56,88,124)."""
    init_model = model.clone()
    adapt_model = model.clone()
    acc = np.zeros((rep_params['n_tasks'], 2))
    layers = [int(layer) for layer in rep_params['layers']]
    reps = {layer: ([], []) for layer in layers}
    for t in range(rep_params['n_tasks']):
        adapt_d, adapt_l, eval_d, eval_l = prepare_batch(tasks.sample(), shots, ways, device)
        for _ in range(rep_params['adapt_steps']):
            train_error = loss(adapt_model(adapt_d), adapt_l)
            train_error = train_error / len(adapt_d)
            adapt_model.adapt(train_error)
            acc[t, 0] = accuracy(adapt_model(eval_d), eval_l).item()
            acc[t, 1] = accuracy(init_model(eval_d), eval_l).item()
        for layer in layers:
            reps[layer][0].append(_device_rep(adapt_model, adapt_d, layer))
            reps[layer][1].append(_device_rep(init_model, adapt_d, layer))
    # the [c*h*w, b] matrix is already the transpose the reference passes: rows = datapoints, columns = the b images
    return acc, {layer: cca(torch.stack(reps[layer][0]), torch.stack(reps[layer][1]), epsilon).mean.cpu().tolist() for layer in layers}
