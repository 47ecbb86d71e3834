"""Generate simulated room impulse responses: ``gen_simu.py --mode rir --stage train|val|test --data_num N --save_to DIR --gpus [0]``
(sar_ssl_amd.roomsim: image-source model on the GPU, the reference's labels and accept test on the host)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sarssl_boot  # noqa: E402,F401
from sar_ssl_amd.roomsim import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
