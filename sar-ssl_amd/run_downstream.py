"""Downstream entry point with the reference's command line (code/run_downstream.py): the simulated-data branch in both stages, and
the real-data training branch of the room-acoustics tasks:

    python run_downstream.py --ds-train --simu-exp --ds-trainmode finetune --ds-task TDOA --ds-nsimroom 8 --time <pretrain tag>
    python run_downstream.py --ds-test --simu-exp --test-mode cal_metric --ds-trainmode finetune --ds-task TDOA --ds-nsimroom 8 --time <tag>
    python run_downstream.py --ds-train --ds-trainmode finetune --ds-task T60 --ds-real-sim-ratio 1 1 --time <pretrain tag>
    python run_downstream.py --ds-train --ds-trainmode finetune --ds-task TDOA --ds-real-sim-ratio 1 1 --time <pretrain tag>

Without ``--simu-exp`` (T60 / DRR / C50 / ABS) every item is synthesised on the GPU from stored RIRs (``RealData``, rirsynth.py); one
cross-validation trial per measured room; everything after the loaders is the same sweep.  TDOA without ``--simu-exp`` reads the LOCATA
corpus ``gen_LOCATA.py`` wrote (``LocataData``, dataset.RandomMicSigDataset): training mixed with the simulated downstream corpus by
``--ds-real-sim-ratio``, validation and test LOCATA only, one trial.  Refused by the option parser (opt.py): that branch while its corpus
is missing (the message holds the command that writes it), TDOA next to another task or on several GPUs without ``--simu-exp``, and
``--ds-test`` without ``--simu-exp``.

``--ds-train``.  Per task and per (trial, batch size, learning rate) of the sweep: train / validate / test every epoch, early stopping on the
smoothed validation loss with one learning-rate decay (code/run_downstream.py:262-308), ensembling of the last five epochs up to
the best one, final test on the large test set, results to the same ``*-lr_bs_tri_result.mat`` file.  Scalars go to a JSONL log
(tensorboardX is absent here).  Same model code, kernels and learner as pretraining, at T = 1.04 s (nt = 64) for TDOA.

``--ds-test`` (code/run_downstream.py:380-534) evaluates what ``--ds-train`` left, see ``ds_test_stage``.
"""
import copy
import json
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
import sarssl_boot  # noqa: E402,F401


TEST_BS = 16                                            # code/run_downstream.py:389


def ds_test_lr_index(lr_set):
    """Index into the sweep's learning rates of the run the test stage reads: the reference hard-wires ``lr_idx = 1``
    (code/run_downstream.py:386).  The build-side ``--ds-lr-set`` may hold one entry only, so: ``min(1, len(lr_set) - 1)``."""
    return min(1, len(lr_set) - 1)


def run_dir(dirs, trainmode, task, num, lr, bs, trial_idx):
    """Directory of one run of the sweep, named as the training branch names it."""
    return (dirs["log_task_" + trainmode].replace("TASK", task).replace("NUM", str(num)).replace("LR", str(lr))
            .replace("BAS", str(bs)).replace("TRI", str(trial_idx)))


def ds_test_data_num(test_mode, num, eval_num=None):
    """Sizes of the two sets (code/run_downstream.py:414-417); ``--ds-eval-num`` replaces the test set's, as for the training
    branch's evaluation sets."""
    n = {"train": num, "test": 4000} if test_mode in ("cal_metric", "cal_metric_wo_info") else {"train": 8000, "test": 8000}
    if eval_num:
        n["test"] = eval_num
    return n


def save_embed(result_dir, stage, run, vis, seed):
    """``embed_<stage>_<run>.mat`` = {'embed' (n, d) f32, 'label' (n, 1)}, always; the reference's ``tsne_vis_<stage>_<run>.png`` / ``.mat``
    (code/run_downstream.py:493-503) when sklearn and matplotlib import, else one line saying so.  -> the names of the files written."""
    import numpy as np
    import scipy.io
    from sar_ssl_amd.common.utils import set_random_seed, vis_TSNE
    embed = vis["embed"].detach().float().cpu().numpy()
    label = vis["label"].detach().float().cpu().numpy()
    files = ["embed_%s_%s.mat" % (stage, run)]
    scipy.io.savemat(os.path.join(result_dir, files[0]), {"embed": embed, "label": label})
    set_random_seed(seed)
    try:
        plt, data_vis = vis_TSNE(data=embed, label=label)
    except ImportError as e:
        print("t-SNE files of the %s set skipped (%s); %s holds the embeddings" % (stage, e, files[0]))
        return files
    stem = "tsne_vis_%s_%s" % (stage, run)
    plt.savefig(os.path.join(result_dir, stem + ".png"))
    plt.close()
    scipy.io.savemat(os.path.join(result_dir, stem + ".mat"), {"data": data_vis["data"], "label": data_vis["label"]})
    return files + [stem + ".png", stem + ".mat"]


def ds_test_stage(args, dirs, net, seeds, selecting, stft):
    """``--ds-test --simu-exp`` (code/run_downstream.py:380-534).  Per task, the run at ``bs_set[0]`` and ``lr_set[ds_test_lr_index(lr_set)]``
    of every trial, on the trial's training directories and the simulated test set, batches of 16 in file order:

      cal_metric           load ensemble_model.tar, test_epoch on the test set: loss and MAE per trial and their mean
      cal_metric_wo_info   no model: the MAE when the mean training target is the prediction (mae_wotrain); mean of the MAEs and
                           means, min of the minima, max of the maxima over the trials
      vis_embed            load ensemble_model.tar, test_epoch(return_vis=True) on both sets: embed_{train,test}_<run>.mat and, with
                           sklearn and matplotlib, tsne_vis_{train,test}_<run>.{png,mat}

    All under ``exp/<TASK>/<time>/test_result/`` (created here; the reference assumes it), with one record per task and mode,
    ``<test_mode>-<trainmode>.json`` = {task, test_mode, lr, bs, trials: [..], mean: {..}}.  One process on the first listed GPU: the stage only
    evaluates and has no data-parallel form.  The evaluation is ``Learner.test_epoch``: full batches replay the captured evaluation step, the
    ragged last one takes its launch-by-launch twin.  Not copied from the reference: its final summary, which formats a list with
    ``{:.4f}`` and raises (the per-task values are printed instead), and its ``'valsim' in dirs[...]`` special case, which never applies
    to the simulated layout."""
    import numpy as np
    import torch
    from sar_ssl_amd import dataset as at_dataset, learner as at_learner
    from sar_ssl_amd.common.utils import set_seed, set_random_seed

    print("Downstream test stage!", args.ds_trainmode)
    print("Number of simulated rooms: ", args.ds_nsimroom)
    mode, fs = args.test_mode, stft["fs"]
    summary = {}
    for task in args.ds_task:
        set_seed(args.seed)
        st = args.ds_setting[task]
        nepoch, num, bs_set, lr_set, ntrials = st["nepoch"], st["num"], st["bs_set"], st["lr_set"], st["ntrial"]
        lr_init, bs = lr_set[ds_test_lr_index(lr_set)], bs_set[0]
        data_num = ds_test_data_num(mode, num, args.ds_eval_num)
        print(task, "nepoch=", nepoch, "num=", num, "lr=", lr_init, "bs=", bs)
        result_dir = os.path.join(dirs["log_task"].replace("TASK", task), "test_result")
        os.makedirs(result_dir, exist_ok=True)
        trials = []
        for trial_idx in range(ntrials):
            print("trial(or cross_validation_dataset)_idx=", trial_idx, "ntrial=", ntrials)
            task_dir = run_dir(dirs, args.ds_trainmode, task, num, lr_init, bs, trial_idx)
            run = os.path.basename(task_dir)
            datasets = {}
            for stage in ("train", "test"):
                key = "micsig_" + stage + "_simu"
                data_dir = dirs[key][trial_idx] if stage == "train" else dirs[key]
                datasets[stage] = at_dataset.FixMicSigDataset(data_dir=data_dir, load_anno=True, load_dp=False, fs=fs,
                                                              dataset_sz=data_num[stage], transforms=[selecting])
            kwargs = {"num_workers": args.workers, "pin_memory": True}
            dl_train = torch.utils.data.DataLoader(datasets["train"], batch_size=TEST_BS, shuffle=False, **kwargs)
            dl_test = torch.utils.data.DataLoader(datasets["test"], batch_size=TEST_BS, shuffle=False, **kwargs)
            learner = at_learner.STFTLearner(net, win_len=stft["win_len"], win_shift_ratio=stft["win_shift_ratio"], nfft=stft["nfft"],
                                             fre_used_ratio=stft["fre_used_ratio"], fs=fs, task=task, ch_mode="M")
            learner.cuda()
            if args.use_amp:
                learner.amp()
            rec = {"trial": trial_idx, "run": run}
            if mode == "cal_metric":
                rec["epochs"] = [int(e) for e in learner.load_checkpoint_ensemble(checkpoints_dir=task_dir)]
                set_random_seed(seeds["test"])
                loss_test, metric_test = learner.test_epoch(dl_test, return_metric=True, return_vis=False)
                rec.update(loss=float(loss_test), metric=float(metric_test))
                print("{} estimation, Test loss: {:.4f}, Test metric: {:.4f}".format(task, rec["loss"], rec["metric"]))
            elif mode == "vis_embed":
                rec["epochs"] = [int(e) for e in learner.load_checkpoint_ensemble(checkpoints_dir=task_dir)]
                set_random_seed(seeds["train"])
                loss_train, metric_train, vis_train = learner.test_epoch(dl_train, return_metric=True, return_vis=True)
                set_random_seed(seeds["test"])
                loss_test, metric_test, vis_test = learner.test_epoch(dl_test, return_metric=True, return_vis=True)
                rec.update(loss_train=float(loss_train), metric_train=float(metric_train), loss=float(loss_test), metric=float(metric_test))
                rec["files"] = (save_embed(result_dir, "train", run, vis_train, seeds["train"])
                                + save_embed(result_dir, "test", run, vis_test, seeds["test"]))
            else:
                names = ("mae_test", "min_test", "max_test", "mae_train", "mean_train", "min_train", "max_train")
                rec.update(zip(names, learner.mae_wotrain(dl_train, dl_test)))
                print("Trial: {}, Data MAE: {:.4f}".format(trial_idx, rec["mae_test"]))
            trials.append(rec)
        how = {"min_test": np.min, "min_train": np.min, "max_test": np.max, "max_train": np.max}
        mean = {k: float(how.get(k, np.mean)([t[k] for t in trials])) for k, v in trials[0].items() if isinstance(v, float)}
        if mode == "cal_metric_wo_info":
            print("Data MAE: {:.4f}".format(mean["mae_test"]))
        else:
            print("{} estimation, Test loss: {:.4f}, Test metric: {:.4f}".format(task, mean["loss"], mean["metric"]))
        with open(os.path.join(result_dir, "%s-%s.json" % (mode, args.ds_trainmode)), "w") as f:
            json.dump({"task": task, "test_mode": mode, "lr": lr_init, "bs": bs, "trials": trials, "mean": mean}, f, indent=1)
        summary[task] = mean
    print("Task: ", args.ds_task)
    for task, mean in summary.items():
        print(task, " ".join("{}: {:.4f}".format(k, v) for k, v in mean.items()))


class RealData:
    """The real-data branch's datasets (code/run_downstream.py:107-110, 132-134, 191-212) for T60 / DRR / C50 / ABS: per task the
    cross-validation trials over the rooms of ``dirs['rir_real']``, per (trial, stage) a rirsynth.RirSynthLoader - training at
    ``--ds-real-sim-ratio`` with the simulated RIRs of ``dirs['rir_train_simu']``, validation and test measured-only, sources from
    ``dirs['srcsig_<stage>']``, seeds[stage] as the datasets' seed.  Banks are built once per directory set and stay resident."""

    def __init__(self, args, dirs, T, fs, seeds, device):
        self.args, self.dirs, self.T, self.fs, self.seeds, self.device = args, dirs, T, fs, seeds, device
        self.ratios = {"train": list(args.ds_specifics["real_sim_ratio"]), "val": [1, 0], "test": [1, 0]}
        self.rooms, self._measured, self._sources, self._simulated = None, {}, {}, None

    def new_task(self):
        from sar_ssl_amd.common.utils import cross_validation_datadir
        self.rooms = cross_validation_datadir(self.dirs["rir_real"])
        return len(self.rooms)

    def loader(self, trial_idx, stage, dataset_sz, batch_size):
        from sar_ssl_amd import rirsynth
        st = stage.split("_")[0]
        ratio, ac = self.ratios[st], self.args.acoustic_setting
        measured = simulated = None
        if ratio[0]:
            key = tuple(self.rooms[trial_idx][st])
            if key not in self._measured:
                self._measured[key] = rirsynth.MeasuredBank(list(key), fs=self.fs)
            measured = self._measured[key]
        if ratio[1]:
            if self._simulated is None:
                self._simulated = rirsynth.SimulatedBank(self.dirs["rir_" + st + "_simu"], fs=self.fs, c=ac["sound_speed"])
            simulated = self._simulated
        if st not in self._sources:
            self._sources[st] = rirsynth.SourceBank(self.dirs["srcsig_" + st], fs=self.fs)
        return rirsynth.RirSynthLoader(measured, simulated, self._sources[st], dataset_sz=dataset_sz, batch_size=batch_size, T=self.T, fs=self.fs,
                                       nmic=ac["nmic"], snr_range=ac["snr_range"], real_sim_ratio=ratio, seed=self.seeds[st],
                                       noise="device", device=self.device, c=ac["sound_speed"])


class LocataData:
    """The real-data branch's datasets for TDOA (code/run_downstream.py:213-230): per stage a dataset.RandomMicSigDataset batch loader over
    the corpus gen_LOCATA.py wrote under ``dirs['micsig_real']`` - training mixed with the simulated segments of
    ``dirs['micsig_train_simu']`` by ``--ds-real-sim-ratio``, validation, test and test_large LOCATA only (``test_large`` reads the
    ``test`` directory, as every ``stage.split('_')[0]`` of the reference does).  One trial."""

    def __init__(self, args, dirs, fs, selecting, device):
        self.dirs, self.fs, self.selecting, self.device = dirs, fs, selecting, device
        self.ratios = {"train": list(args.ds_specifics["real_sim_ratio"]), "val": [1, 0], "test": [1, 0]}

    def new_task(self):
        return 1

    def loader(self, trial_idx, stage, dataset_sz, batch_size):
        from sar_ssl_amd import dataset as at_dataset
        st = stage.split("_")[0]
        return at_dataset.RandomMicSigDataset(real_sig_dir=self.dirs["micsig_real"],
                                              sim_sig_dir=self.dirs["micsig_" + st + "_simu"] if stage == "train" else [],
                                              real_sim_ratio=self.ratios[st], fs=self.fs, stage=st, load_anno=True, dataset_sz=dataset_sz,
                                              transforms=[self.selecting], batch_size=batch_size, device=self.device)


def main(argv=None):
    from sar_ssl_amd.opt import opt_downstream
    opts = opt_downstream()
    args = opts.parse(argv)
    dirs = opts.dir()
    if "LOCAL_RANK" not in os.environ:
        os.environ["HIP_VISIBLE_DEVICES"] = ",".join(g for g in args.gpu_id.split(",") if g != "")

    import numpy as np
    import scipy.io
    import torch
    from sar_ssl_amd import dataset as at_dataset, learner as at_learner, model as at_model
    from sar_ssl_amd.common.utils import set_seed, set_random_seed, get_nparams

    if args.no_cuda or not torch.cuda.is_available():
        raise SystemExit("run_downstream.py (sar_ssl_amd) needs an MI355X GPU: the HIP path has no CPU fallback")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    set_seed(args.seed)
    assert args.source_state == "static", "Source state model unrecognized~"
    fs = args.acoustic_setting["fs"]
    seeds = {"train": int(args.seed + 2e8), "val": int(args.seed + 1e8), "test": int(args.seed + 1)}
    T = 1.04 if args.ds_task == ["TDOA"] else 4.112                                         # code/run_downstream.py:67-70
    selecting = at_dataset.Selecting(select_range=[0, int(T * fs)])
    win_len, nfft, win_shift_ratio, fre_used_ratio = 512, 512, 0.5, 1
    nf = nfft // 2
    nt = int((T * fs - win_len * (1 - win_shift_ratio)) / (win_len * win_shift_ratio))
    net = at_model.SARSSL(sig_shape=(nf, nt, 2, 2), pretrain=False, device=device, downstream_token=args.ds_token,
                          downstream_head=args.ds_head, downstream_embed=args.ds_embed, downstream_dlabel=1)
    nparam, nparam_sum = get_nparams(net, param_key_list=["spec_encoder", "spat_encoder", "mlp_head"])
    print("duration:", T, "s; nt, nf:", nt, nf, "; # Parameters (M):", round(nparam_sum, 2))
    if args.ds_test:
        return ds_test_stage(args, dirs, net, seeds, selecting,
                          dict(win_len=win_len, win_shift_ratio=win_shift_ratio, nfft=nfft, fre_used_ratio=fre_used_ratio, fs=fs))

    log_dir = "log_task_" + args.ds_trainmode
    init_state_dict = copy.deepcopy(net.state_dict())
    real = None
    if not args.simu_exp:
        real = (LocataData(args, dirs, fs, selecting, device) if args.ds_specifics["data"] == "real_locata"
                else RealData(args, dirs, T, fs, seeds, device))
    for task in args.ds_task:
        set_seed(args.seed)
        task_time_dir = dirs["log_task"].replace("TASK", task)
        st = args.ds_setting[task]
        nepoch, num, bs_set, lr_set, ntrials = st["nepoch"], st["num"], st["bs_set"], st["lr_set"], st["ntrial"]
        if real is not None:
            ntrials = real.new_task()                       # one trial per room (code/run_downstream.py:132-134)
        neval = args.ds_eval_num
        data_num = {"train": num, "val": neval or 1000, "test": neval or 1000, "test_large": neval or 4000}
        stages = ["train", "val", "test", "test_large"]
        test_bs, early_stop_patience, smooth_alpha, nepoch_ensemble, num_stop_th = 16, 10, 0.6, 5, 1
        nlrs, nbss = len(lr_set), len(bs_set)
        shape = (nlrs, nbss, ntrials)
        val_losses, test_losses, val_metrics, test_metrics = (np.zeros(shape) for _ in range(4))
        ensemble_epochs = np.zeros(shape + (2,))
        os.makedirs(task_time_dir, exist_ok=True)
        task_dir = None
        for trial_idx in range(ntrials):
            for bs_idx in range(nbss):
                for lr_idx in range(nlrs):
                    set_seed(args.seed)
                    lr_init, bs = lr_set[lr_idx], bs_set[bs_idx]
                    print(task, ": nepoch=", nepoch, "num=", num, "lr=", lr_init, "bs=", bs, "trial_idx=", trial_idx, "ntrial=", ntrials)
                    task_dir = (dirs[log_dir].replace("TASK", task).replace("NUM", str(num)).replace("LR", str(lr_init))
                                .replace("BAS", str(bs)).replace("TRI", str(trial_idx)))
                    os.makedirs(task_dir, exist_ok=True)
                    datasets = {}
                    for stage in stages if real is None else ():
                        key = "micsig_" + stage.split("_")[0] + "_simu"
                        data_dir = dirs[key][trial_idx] if stage == "train" else dirs[key]
                        datasets[stage] = at_dataset.FixMicSigDataset(data_dir=data_dir, load_anno=True, load_dp=False, fs=fs,
                                                                      dataset_sz=data_num[stage], transforms=[selecting])
                    kwargs = {"num_workers": args.workers, "pin_memory": True}
                    if real is not None:
                        dl_train, dl_val, dl_test, dl_test_large = (real.loader(trial_idx, stage, data_num[stage], bs if stage == "train" else test_bs)
                                                                    for stage in stages)
                    else:
                        dl_train = torch.utils.data.DataLoader(datasets["train"], batch_size=bs, shuffle=True, **kwargs)
                        dl_val = torch.utils.data.DataLoader(datasets["val"], batch_size=test_bs, shuffle=False, **kwargs)
                        dl_test = torch.utils.data.DataLoader(datasets["test"], batch_size=test_bs, shuffle=False, **kwargs)
                        dl_test_large = torch.utils.data.DataLoader(datasets["test_large"], batch_size=test_bs, shuffle=False, **kwargs)

                    net.load_state_dict(init_state_dict)
                    for p in net.parameters():
                        p.requires_grad = True
                    learner = at_learner.STFTLearner(net, win_len=win_len, win_shift_ratio=win_shift_ratio, nfft=nfft,
                                                     fre_used_ratio=fre_used_ratio, fs=fs, task=task, ch_mode="M")
                    learner.cuda()
                    if args.use_amp:
                        learner.amp()
                    if args.checkpoint_start:
                        learner.resume_checkpoint(checkpoints_dir=task_dir, from_latest=True, as_all_state=True)
                    elif args.ds_trainmode == "finetune":
                        learner.load_checkpoint_best(checkpoints_dir=dirs["log_pretrain"], as_all_state=False, param_frozen=False)
                    elif args.ds_trainmode == "lineareval":
                        learner.load_checkpoint_best(checkpoints_dir=dirs["log_pretrain"], as_all_state=False, param_frozen=True)

                    log = open(os.path.join(task_dir, "scalars.jsonl"), "a")
                    loss_val_list, lr, cnt_stop, best_epoch, epoch = [], lr_init * 1, 0, learner.start_epoch, learner.start_epoch
                    for epoch in range(learner.start_epoch, nepoch + 1):
                        set_random_seed(seeds["train"])
                        loss_train, metric_train = learner.train_epoch(dl_train, lr=lr, epoch=epoch, return_metric=True)
                        set_random_seed(seeds["val"])
                        loss_val, metric_val = learner.test_epoch(dl_val, return_metric=True)
                        set_random_seed(seeds["test"])
                        loss_test, metric_test = learner.test_epoch(dl_test, return_metric=True)
                        loss_val_list += [loss_val]
                        smooth = learner.smooth_data(data_list=loss_val_list, alpha=smooth_alpha)
                        stop_flag, is_best = learner.early_stopping(current_score=smooth[-1] * (-1), patience=early_stop_patience)
                        learner.save_checkpoint(epoch=epoch, checkpoints_dir=task_dir, is_best_epoch=is_best, save_extra_hist=True)
                        if is_best:
                            best_epoch = copy.deepcopy(epoch)
                        rec = {"epoch": epoch, "lr": lr, "loss_train": loss_train, "metric_train": float(metric_train),
                               "loss_val": loss_val, "metric_val": float(metric_val), "loss_val_smooth": smooth[-1],
                               "loss_test": loss_test, "metric_test": float(metric_test)}
                        print(json.dumps(rec), flush=True)
                        log.write(json.dumps(rec) + "\n"); log.flush()
                        if stop_flag:
                            cnt_stop += 1
                            if cnt_stop <= num_stop_th:
                                lr = lr / 10
                                print("lr decaing")
                                learner.early_stop_counter = 0
                            else:
                                break
                    print("\nTraining finished\n")
                    st_epoch = int(np.maximum(1, best_epoch - nepoch_ensemble + 1))
                    ed_epoch = copy.deepcopy(best_epoch)
                    learner.ensembling(checkpoints_dir=task_dir, epochs=[i for i in range(st_epoch, ed_epoch + 1)])
                    set_random_seed(seeds["test"])
                    best_loss_test, best_metric_test = learner.test_epoch(dl_test_large, return_metric=True)
                    set_random_seed(seeds["val"])
                    best_loss_val, best_metric_val = learner.test_epoch(dl_val, return_metric=True)
                    print("{} estimation, Test loss: {:.4f}, Test metric: {:.4f}".format(task, best_loss_test, float(best_metric_test)))
                    print("{} estimation, Val loss: {:.4f}, Val metric: {:.4f}".format(task, best_loss_val, float(best_metric_val)))
                    learner.remove_checkpoint_epochs(checkpoints_dir=task_dir, epochs=[i for i in range(1, st_epoch)] +
                                                     [i for i in range(best_epoch + 1, epoch + 1)])
                    val_losses[lr_idx, bs_idx, trial_idx], val_metrics[lr_idx, bs_idx, trial_idx] = best_loss_val, float(best_metric_val)
                    test_losses[lr_idx, bs_idx, trial_idx], test_metrics[lr_idx, bs_idx, trial_idx] = best_loss_test, float(best_metric_test)
                    ensemble_epochs[lr_idx, bs_idx, trial_idx, :] = [st_epoch, ed_epoch]
                    log.close()
        metric = np.mean(val_metrics, axis=-1)
        idxes = metric.argmin()
        best_lr_idx, best_bs_idx = idxes // metric.shape[1], idxes % metric.shape[1]
        print("\n{} estimation, BS: {}, LR: {}, best val MAE: {:.4f}, best test MAE: {:.4f}\n".format(
            task, bs_set[best_bs_idx], lr_set[best_lr_idx], metric[best_lr_idx, best_bs_idx],
            np.mean(test_metrics, axis=-1)[best_lr_idx, best_bs_idx]))
        atts = task_dir.replace(task_time_dir, "").split("-")
        result_name = "-".join([atts[0], atts[1], atts[2], atts[3], atts[-2], atts[-1]]) + "-lr_bs_tri_result.mat"
        scipy.io.savemat(task_time_dir + "/" + result_name.lstrip("/"), {
            "val_losses": val_losses, "val_metrics": val_metrics, "test_losses": test_losses, "test_metrics": test_metrics,
            "lr_set": lr_set, "bs_set": bs_set, "ntrial": ntrials, "best_lr_idx": best_lr_idx, "best_bs_idx": best_bs_idx,
            "ensemble_epoch": ensemble_epochs})


if __name__ == "__main__":
    main()
