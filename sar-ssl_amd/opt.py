"""Command-line options and directory layouts of the entry points: same flag names / defaults as ``opt_pretrain``
(code/opt.py:6-115) and ``opt_downstream`` (code/opt.py:117-320: the simulated-data branch and the real-data branch - T60 / DRR / C50 /
ABS on signals synthesised from stored RIRs, TDOA on the LOCATA corpus ``gen_LOCATA.py`` writes) in the reference."""
import argparse
import os
import time

import numpy as np


class opt_pretrain():
    REFUSE_ONLINE = ("--simu-online (with --simu-online-reuse / --simu-online-bank-gb) renders the TRAINING batches of simulated pretraining "
                     "on the GPU and is valid only with `--pretrain --simu-exp`; this command has %s (validation, --test and "
                     "--pretrain-frozen-encoder read their corpora from disk)")

    def __init__(self):
        self.time = time.strftime("%m%d%H%M", time.localtime(time.time()))
        self.work_dir = os.path.abspath(os.path.expanduser(r"~"))
        self.work_dir_local = self.work_dir
        self.acoustic_setting = {"sound_speed": 343.0, "fs": 16000, "T": 4.112, "nmic": 2, "mic_dist_range": [0.03, 0.20]}
        self.simu_exp = False

    def parse(self, argv=None):
        p = argparse.ArgumentParser(description="Self-supervised learing for multi-channel audio processing")
        p.add_argument("--gpu-id", type=str, default="7", metavar="GPU", help="GPU ID (default: 7)")
        p.add_argument("--workers", type=int, default=8, metavar="Worker", help="number of workers (default: 8)")
        p.add_argument("--bs", type=int, nargs="+", default=[128, 128, 128], metavar="TrainValTestBatch",
                       help="batch size for training, validation and test (default: [128, 128, 128])")
        p.add_argument("--no-cuda", action="store_true", default=False, help="disables CUDA training (default: False)")
        p.add_argument("--use-amp", action="store_true", default=False, help="Use mixed precision (MI355X: the 'hybrid' mode - fp16 stem, f32 residual stream; SARSSL_AMP_DTYPE=fp16|bf16 selects the others)")
        p.add_argument("--seed", type=int, default=1, metavar="Seed", help="random seed (default: 1)")
        p.add_argument("--checkpoint-start", action="store_true", default=False, help="train model from saved latest checkpoints")
        p.add_argument("--checkpoint-from-best-epoch", action="store_true", default=False, help="train model from saved best checkpoints")
        p.add_argument("--time", type=str, default=self.time, metavar="Time", help="time flag")
        p.add_argument("--work-dir", type=str, default=self.work_dir, metavar="WorkDir", help="work directory")
        p.add_argument("--sources", type=int, nargs="+", default=[1], metavar="Sources", help="number of sources (default: 1)")
        p.add_argument("--source-state", type=str, default="static", metavar="SourceState", help="state of sources")
        p.add_argument("--simu-exp", action="store_true", default=False, help="Experiments on simulated data")
        p.add_argument("--pretrain", action="store_true", default=False, help="change to pretrain stage")
        p.add_argument("--pretrain-frozen-encoder", action="store_true", default=False, help="second stage: load the encoders of the pretraining run (exp/pretrain/<time>/best_model.tar), freeze them and train a fresh "
                            "decoder to reconstruct the masked channel (single GPU; checkpoints under exp/pretrain_frozen_encoder/<time>)")
        p.add_argument("--nepoch", type=int, default=30, metavar="Epoch", help="number of epochs to train (default: 30)")
        p.add_argument("--lr", type=float, default=0.001, metavar="LR", help="learning rate (default:0.001)")
        p.add_argument("--test", action="store_true", default=False, help="change to test stage")
        p.add_argument("--test-mode", type=str, default="all", metavar="TestMode", help="test mode (default: all)")
        p.add_argument("--data-num", type=int, nargs=2, default=None, metavar=("Train", "Val"),
                       help="items per epoch and per validation of real-data pretraining (build-side override for a short run; "
                            "default: the reference's 512000 and 8000)")
        p.add_argument("--simu-online", action="store_true", default=False,
                       help="with --pretrain --simu-exp: render every training batch on the GPU while the previous step runs "
                            "(onlinesig.OnlineSignalLoader over <work-dir>/data/SrcSig/wsj0/tr) instead of reading MicSig/simu/pretrain; "
                            "nothing is written and no room repeats; --data-num sets the items per epoch; validation reads preval from disk")
        p.add_argument("--simu-online-reuse", type=int, default=1, metavar="K",
                       help="--simu-online: every rendered room serves K consecutive items that differ in source, noise and SNR "
                            "(K divides the training batch size; default: 1)")
        p.add_argument("--simu-online-bank-gb", type=float, default=8.0, metavar="G",
                       help="--simu-online: the most the source corpus may take on the device, in GiB; a larger corpus is refused, "
                            "never truncated (default: 8)")
        args = p.parse_args(argv)
        assert (args.pretrain + args.pretrain_frozen_encoder + args.test) == 1, "Pretraining stage (pretrain or test) is undefined"
        assert args.test_mode in ["all", "ins"], "Test mode is undefined"
        online = args.simu_online or args.simu_online_reuse != 1 or args.simu_online_bank_gb != 8.0
        if online and (args.test or args.pretrain_frozen_encoder or not args.simu_exp):
            raise SystemExit(self.REFUSE_ONLINE % ("--test" if args.test else "--pretrain-frozen-encoder" if args.pretrain_frozen_encoder
                                                   else "no --simu-exp"))
        if online and not args.simu_online:
            raise SystemExit("--simu-online-reuse / --simu-online-bank-gb set what --simu-online renders: give --simu-online with them")
        if args.simu_online_reuse < 1 or args.bs[0] % args.simu_online_reuse != 0:
            raise SystemExit("--simu-online-reuse %d does not divide the training batch size %d: the items of a room share one batch"
                             % (args.simu_online_reuse, args.bs[0]))
        self.time, self.work_dir = args.time, os.path.abspath(os.path.expanduser(args.work_dir))
        self.work_dir_local = self.work_dir
        self.simu_exp = bool(args.simu_exp)
        args.acoustic_setting = self.acoustic_setting
        return args

    def dir(self):
        work_dir = self.work_dir
        dirs = {"code": work_dir + "/SAR-SSL/code", "data": self.work_dir_local + "/data",
                "gerdata": self.work_dir_local + "/SAR-SSL/data", "exp": work_dir + "/SAR-SSL/exp"}
        dirs["micsig_simu_pretrain"] = dirs["gerdata"] + "/MicSig/simu/pretrain"
        dirs["micsig_simu_preval"] = dirs["gerdata"] + "/MicSig/simu/preval"
        dirs["micsig_simu_pretest"] = dirs["gerdata"] + "/MicSig/simu/pretest"
        dirs["micsig_simu_pretest_ins"] = [dirs["gerdata"] + "/MicSig/simu/pretest_ins_T1000"]
        dirs["srcsig_train"] = dirs["data"] + "/SrcSig/wsj0/tr"                                    # --simu-online's sources (code/opt.py:273)
        if not self.simu_exp:                                                                    # code/opt.py:82-109
            real, rec = dirs["gerdata"] + "/MicSig/real/", dirs["data"] + "/MicSig/"
            recordings = {"LOCATA": rec + "LOCATA", "MCWSJ": rec + "MC_WSJ_AV", "LibriCSS": rec + "LibriCSS", "AMI": rec + "AMI",
                          "AISHELL4": rec + "AISHELL-4", "M2MeT": rec + "M2MeT", "RealMAN": rec + "RealMAN",
                          "RealMANOri": rec + "aligned_static_high_\u7cbe\u7ec6\u5bf9\u9f50_correctDPRIR_filtered3"}
            dirs["micsig_real_pretrain"] = {n: real + "pretrain/" + n for n in ("DCASE", "MIR", "Mesh", "BUTReverb", "dEchorate", "ACE")}
            dirs["micsig_real_pretrain"].update(recordings)
            dirs["micsig_real_preval"] = {n: real + "preval/" + n for n in ("DCASE", "BUTReverb")}
            dirs["micsig_real_preval"].update({n: recordings[n] for n in ("AISHELL4", "M2MeT", "RealMAN", "RealMANOri")})
            dirs["micsig_real_pretest"] = {"ACE": real + "pretrain/ACE", "LOCATA": recordings["LOCATA"]}
        dirs["log_pretrain"] = dirs["exp"] + "/pretrain/" + self.time
        dirs["log_pretrain_frozen_encoder"] = dirs["exp"] + "/pretrain_frozen_encoder/" + self.time            # code/opt.py:113
        return dirs


class opt_downstream():
    """Downstream (TDOA / DRR / C50 / T60 / ABS regression on the pretrained encoders) options: the simulated-data branch (--simu-exp) and
    the real-data branch: the room-acoustics tasks on signals synthesised from stored RIRs (rirsynth.py), TDOA on the LOCATA corpus
    (locatads.py, dataset.RandomMicSigDataset).
    ``--ds-nepoch/--ds-num/--ds-lr-set/--ds-bs-set/--ds-eval-num`` are build-side overrides of the reference's hard-wired sweep
    (code/opt.py:197-209) so that a short run is possible; left unset, the reference's values apply."""

    def __init__(self):
        self.time = time.strftime("%m%d%H%M", time.localtime(time.time()))
        self.work_dir = os.path.abspath(os.path.expanduser(r"~"))
        self.work_dir_local = self.work_dir
        self.acoustic_setting = {"sound_speed": 343.0, "fs": 16000, "snr_range": [15, 30], "nmic": 2, "mic_dist_range": [0.03, 0.20]}
        self.extra_info, self.ds_token, self.ds_head, self.ds_embed, self.ds_nsimroom = "", "", "", "", 0
        self.simu_exp, self.ntrail, self.ds_specifics = True, 1, {}

    def parse(self, argv=None):
        p = argparse.ArgumentParser(description="Self-supervised learing for multi-channel audio processing")
        p.add_argument("--gpu-id", type=str, default="6,", metavar="GPU", help="GPU ID")
        p.add_argument("--workers", type=int, default=4, metavar="Worker", help="number of workers (default: 4)")
        p.add_argument("--no-cuda", action="store_true", default=False)
        p.add_argument("--use-amp", action="store_true", default=False, help="mixed precision (the 'hybrid' mode; SARSSL_AMP_DTYPE=fp16|bf16 selects the others)")
        p.add_argument("--seed", type=int, default=1, metavar="Seed")
        p.add_argument("--checkpoint-start", action="store_true", default=False)
        p.add_argument("--time", type=str, default=self.time, metavar="Time")
        p.add_argument("--work-dir", type=str, default=self.work_dir, metavar="WorkDir")
        p.add_argument("--sources", type=int, nargs="+", default=[1])
        p.add_argument("--source-state", type=str, default="static")
        p.add_argument("--simu-exp", action="store_true", default=False)
        p.add_argument("--ds-train", action="store_true", default=False)
        p.add_argument("--ds-trainmode", type=str, default="finetune")
        p.add_argument("--ds-task", type=str, nargs="+", default=["TDOA"])
        p.add_argument("--ds-token", type=str, default="all")
        p.add_argument("--ds-head", type=str, default="mlp")
        p.add_argument("--ds-embed", type=str, default="spat")
        p.add_argument("--ds-nsimroom", type=int, default=0)
        p.add_argument("--ds-real-sim-ratio", type=int, nargs="+", default=[1, 1])
        p.add_argument("--ds-test", action="store_true", default=False)
        p.add_argument("--test-mode", type=str, default="cal_metric_wo_info")
        p.add_argument("--ds-nepoch", type=int, default=None)
        p.add_argument("--ds-num", type=int, default=None)
        p.add_argument("--ds-lr-set", type=float, nargs="+", default=None)
        p.add_argument("--ds-bs-set", type=int, nargs="+", default=None)
        p.add_argument("--ds-eval-num", type=int, default=None, help="size of the val / test sets (reference: 1000, test_large 4000)")
        args = p.parse_args(argv)
        assert (args.ds_train + args.ds_test) == 1, "Downstream stage (train or test) is not defined"
        assert args.ds_trainmode in ["scratchLOW", "finetune", "lineareval"], "Downstream train mode in not defined"
        assert args.test_mode in ["cal_metric", "cal_metric_wo_info", "vis_embed"], "Test mode is undefined"
        self.simu_exp, self.time = args.simu_exp, args.time
        self.work_dir = os.path.abspath(os.path.expanduser(args.work_dir))
        self.work_dir_local = self.work_dir
        self.ds_token, self.ds_head, self.ds_embed, self.ds_nsimroom = args.ds_token, args.ds_head, args.ds_embed, args.ds_nsimroom
        self.ds_specifics = args.ds_specifics = {"task": args.ds_task}
        args.acoustic_setting = self.acoustic_setting
        if not self.simu_exp:
            return self._parse_real(args)
        bs_set = args.ds_bs_set or [8]
        lr_set = args.ds_lr_set or [0.001, 0.0005, 0.0001, 0.00005]
        nepoch = args.ds_nepoch or 200
        num = args.ds_num if args.ds_num is not None else args.ds_nsimroom * 100
        ntrial = int(np.maximum(1, round(32 / (args.ds_nsimroom + 10e-4))))
        self.ntrail = ntrial
        args.ds_setting = {t: {"nepoch": nepoch, "num": num, "lr_set": lr_set, "bs_set": bs_set, "ntrial": ntrial}
                           for t in ("TDOA", "DRR", "C50", "T60", "ABS")}
        self.extra_info = "R" + str(args.ds_nsimroom)
        return args

    REFUSE_TDOA_REAL = ("the LOCATA TDOA real-data branch (RandomMicSigDataset, code/run_downstream.py:213-230) reads the pre-generated "
                        "corpus %s/{train,val,test}/{idx}.wav + {idx}_info.npz, and %s/train holds no segment.  Write it with\n"
                        "  python gen_LOCATA.py --stage train val test --data-dir <data>/MicSig/LOCATA --save-to %s\n"
                        "(TDOA also runs on simulated data with --simu-exp; without it T60, DRR, C50 and ABS run on signals synthesised "
                        "from stored RIRs)")
    REFUSE_TDOA_MIXED = ("--ds-task TDOA together with %s: on real data TDOA trains on the LOCATA corpus at T = 1.04 s and the "
                         "room-acoustics tasks on signals synthesised from stored RIRs at T = 4.112 s - run them one after the other")
    REFUSE_TEST_REAL = ("--ds-test is simulated-only, as in the reference (code/run_downstream.py:383 asserts --simu-exp): "
                        "`--ds-test --simu-exp` evaluates what `--ds-train --simu-exp` left")

    def _parse_real(self, args):
        """The reference's real-data settings (code/opt.py:189-256): batch 16, two learning rates, the training-set size by train mode and
        real / simulated ratio; the cross-validation trials are counted by run_downstream from the rooms on disk."""
        if args.ds_test:
            raise SystemExit(self.REFUSE_TEST_REAL)
        locata = "TDOA" in args.ds_task
        if locata:
            if len(args.ds_task) > 1:
                raise SystemExit(self.REFUSE_TDOA_MIXED % ", ".join(t for t in args.ds_task if t != "TDOA"))
            if len([g for g in args.gpu_id.split(",") if g != ""]) > 1:
                raise SystemExit("--gpu-id %s: the LOCATA TDOA branch runs on one GPU (data-parallel downstream is not built)" % args.gpu_id)
            corpus = self.work_dir_local + "/SAR-SSL/data/MicSig/real_ds_locata"                 # dir()'s micsig_real
            train = os.path.join(corpus, "train")
            if not (os.path.isdir(train) and any(f.endswith(".wav") for f in os.listdir(train))):
                raise SystemExit(self.REFUSE_TDOA_REAL % (corpus, corpus, corpus))
        ratio = list(args.ds_real_sim_ratio)
        assert ratio in [[0, 1], [1, 0], [1, 1]], ratio                                          # code/dataset.py:262, 358
        self.ds_specifics.update(data="real_locata" if locata else "real_ace", real_sim_ratio=ratio)   # code/opt.py:190-195
        table = {"finetune": {(1, 0): 1600, (1, 1): 3200, (0, 1): 32000}, "scratchLOW": {(1, 0): 1600, (1, 1): 16000, (0, 1): 32000}}
        if args.ds_trainmode not in table:
            raise Exception("Undefined trainmode for the number of real-world training data")
        num = args.ds_num if args.ds_num is not None else table[args.ds_trainmode][tuple(ratio)]
        st = {"nepoch": args.ds_nepoch or 200, "lr_set": args.ds_lr_set or [0.001, 0.0001], "bs_set": args.ds_bs_set or [16], "ntrial": 1}
        args.ds_setting = {t: dict(st, num=num) for t in ("DRR", "C50", "T60", "ABS")}
        args.ds_setting["TDOA"] = dict(st, num=args.ds_num if args.ds_num is not None else 80000)
        return args

    def dir(self):
        work_dir = self.work_dir
        dirs = {"code": work_dir + "/SAR-SSL/code", "data": self.work_dir_local + "/data",
                "gerdata": self.work_dir_local + "/SAR-SSL/data", "exp": work_dir + "/SAR-SSL/exp"}
        if self.simu_exp:
            dirs["micsig_train_simu"] = []
            train_dir = dirs["gerdata"] + "/MicSig/simu_ds/train"
            for trail_idx in range(self.ntrail):
                dirs["micsig_train_simu"] += [[os.path.join(train_dir, "R" + str(trail_idx * self.ds_nsimroom + r + 1))
                                               for r in range(self.ds_nsimroom)]]
            dirs["micsig_val_simu"] = dirs["gerdata"] + "/MicSig/simu_ds/val"
            dirs["micsig_test_simu"] = dirs["gerdata"] + "/MicSig/simu_ds/test"
            flag = "sim_"
        else:                                                                                    # code/opt.py:273-275, 298-308
            dirs["srcsig_train"] = dirs["data"] + "/SrcSig/wsj0/tr"
            dirs["srcsig_val"] = dirs["data"] + "/SrcSig/wsj0/dt"
            dirs["srcsig_test"] = dirs["data"] + "/SrcSig/wsj0/et"
            dirs["rir_real"] = dirs["gerdata"] + "/RIR/real/ACE"
            dirs["rir_train_simu"] = dirs["gerdata"] + "/RIR/simu/train"
            dirs["micsig_real"] = dirs["gerdata"] + "/MicSig/real_ds_locata"                      # LOCATA TDOA: code/opt.py:303-306
            dirs["micsig_train_simu"] = dirs["gerdata"] + "/MicSig/simu_ds/train"
            r = self.ds_specifics["real_sim_ratio"]
            flag = "real_train" + str(r[0]) + "real" + str(r[1]) + "sim_valreal"
        dirs["log_pretrain"] = dirs["exp"] + "/pretrain/" + self.time
        dirs["log_task"] = dirs["exp"] + "/TASK/" + self.time
        for mode, name in (("scratchLOW", "scratchlow"), ("finetune", "finetune"), ("lineareval", "lineareval")):
            dirs["log_task_" + mode] = (dirs["log_task"] + "/" + name + "-" + self.ds_token + "-" + self.ds_head + "-NUM-LR-BAS-TRI-"
                                        + self.ds_embed + "-" + flag + self.extra_info)
        return dirs
