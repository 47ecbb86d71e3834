"""Cut a measured RIR corpus into microphone pairs (sar_ssl_amd.realrir; polyphase resampling on the GPU):
``gen_real_rir.py --dataset ACE --data_type rir noise --fs 16000 --read_dir ../data/RIR --save_dir data/RIR/real [--gpus [0]]`` reads
``<read_dir>/ACE`` and writes the pairs' RIRs with their labels to ``<save_dir>/ACE/<room>/<array>/SP1_MP<pos>-<i>-<j>.npy`` + ``_info.npz``
and the noise cuts to ``<save_dir>/ACE_noise/<room>/<array>/_MP<pos>-<i>-<j>_<type>.wav`` (PCM-16) - the bank rirsynth.MeasuredBank reads."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sarssl_boot  # noqa: E402,F401
from sar_ssl_amd.realrir import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
