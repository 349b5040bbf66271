#!/usr/bin/env python3
"""Drop-in for upstream's ``python3 yolov5/val.py --data DATA.yaml --weights W.pt`` (the table yolov5/train.py prints after every epoch,
reference README.md's training step): P, R, mAP@0.5 and mAP@0.5:0.95 of a set of weights on a labelled split.

Same path, same flags, upstream's table on stdout; the engine, the label matching and the scores run on the MI355X (aquaculture_amd.val).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# as yolov5/detect.py: the CPU side wants no OpenMP / BLAS thread teams; the libraries read these when they are loaded
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, os.environ.get("AQ_CPU_THREADS", "1"))

from aquaculture_amd.val import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
