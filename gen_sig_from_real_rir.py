"""Microphone signals from measured RIR banks, the measured-RIR corpora of real-data pretraining (sar_ssl_amd.realsig; rendered on the GPU):
``gen_sig_from_real_rir.py --stage pretrain|preval --dataset DCASE MIR Mesh dEchorate BUTReverb ACE --src_dir data/SrcSig/wsj0 --rir_dir
data/RIR/real --save_dir data/MicSig/real [--data_num N] [--gpus [0]] [--batch 16]`` reads the banks ``<rir_dir>/<dataset>`` (and their noise
cuts ``<dataset>_noise``) and the sources ``<src_dir>/tr`` or ``/dt``, and writes ``<save_dir>/<stage>/<dataset>/{idx}.wav`` (PCM-16) - what
``run_pretrain.py --pretrain`` without ``--simu-exp`` reads."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sarssl_boot  # noqa: E402,F401
from sar_ssl_amd.realsig import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
