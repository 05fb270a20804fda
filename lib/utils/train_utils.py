"""reference lib/utils/train_utils.py — the checkpoint-ingest part of the tracking path (`load_pretrain`, `remove_prefix`,
`check_keys`) and `is_valid_number`, the loss guard of the training loop: its host form lives beside the optimiser
(usot_amd/optim.py), whose HIP step applies the same rule to the loss on the device.  Schedulers, loggers and checkpoint
writers are out of scope."""
from usot_amd.io_utils import check_keys, load_pretrain, remove_prefix  # noqa: F401
from usot_amd.optim import is_valid_number  # noqa: F401
