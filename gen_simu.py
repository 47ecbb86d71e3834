"""Generate simulated room impulse responses or microphone signals (sar_ssl_amd.roomsim: image-source model on the GPU):
``gen_simu.py --mode rir --stage train|val|test --data_num N --save_to DIR --gpus [0] [--labels host|device]`` writes an RIR bank,
``gen_simu.py --mode sig --stage pretrain|preval|pretest --data_num N --src_dir WSJ0 --save_to DIR --gpus [0]`` the pretraining corpus
(``{idx}.wav`` PCM-16 and ``{idx}_info.npz``; accept test, noise, mix and PCM conversion on the GPU)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sarssl_boot  # noqa: E402,F401
from sar_ssl_amd.roomsim import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
