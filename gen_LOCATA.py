"""The LOCATA TDOA corpus of the downstream task (sar_ssl_amd.locatads; resampled, normalised and labelled on the GPU):
``gen_LOCATA.py --stage train val test --data-dir data/MicSig/LOCATA --save-to data/MicSig/real_ds_locata [--data-num N] [--gpus [0]]
[--batch 16] [--sort] [--overwrite]`` reads the recordings ``<data-dir>/{eval,dev}/task{1,3,5}/<recording>/<array>`` and writes
``<save-to>/<stage>/{idx}.wav`` (1.04 s, two microphones, 16 kHz PCM-16) and ``{idx}_info.npz`` (TDOA).  A stage directory that holds
files already is refused without ``--overwrite``."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sarssl_boot  # noqa: E402,F401
from sar_ssl_amd.locatads import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
