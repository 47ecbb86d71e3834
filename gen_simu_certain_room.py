"""Generate simulated room impulse responses or microphone signals of a fixed number of rooms (sar_ssl_amd.roomsim: image-source model
on the GPU), the data of the downstream stages:
``gen_simu_certain_room.py --mode rir --stage train|val|test --room_num N --save_to DIR --gpus [0]`` writes ``DIR/<stage>/R1 .. RN`` as RIR banks,
``gen_simu_certain_room.py --mode sig --stage train|val|test --room_num N --sig_num_each_rir K --src_dir WSJ0 --save_to DIR --gpus [0]``
the corpus ``run_downstream.py --ds-train --simu-exp`` reads (``R<n>/{i}.wav`` PCM-16 and ``{i}_info.npz``)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sarssl_boot  # noqa: E402,F401
from sar_ssl_amd.roomsim import main_certain_room  # noqa: E402

if __name__ == "__main__":
    sys.exit(main_certain_room())
