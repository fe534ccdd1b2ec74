"""From dry sources to rooms the path can enhance, on the GPU (the reference's disco_theque/dataset_utils/signal_setups.py,
dataset_generation/gen_disco/convolve_signals.py, dataset_generation/gen_meetit/convolve_signals.py and
disco_theque/dataset_utils/post_generator.py, without files and without redraw loops)."""
from .meetings import get_value_range, meeting_masks, meeting_rooms, simulate_meetings, sir_at_nodes, sir_valid
from .post import get_directory_name, get_dset, post_process_rooms, write_post_dataset
from .rooms import mix_rooms, reverb_at_mics, simulate_rooms, snr_at_mics
from .signals import noise_segments, ssn_segments, target_segments

__all__ = ['snr_at_mics', 'simulate_rooms', 'mix_rooms', 'reverb_at_mics', 'target_segments', 'noise_segments', 'ssn_segments',
           'simulate_meetings', 'sir_at_nodes', 'sir_valid', 'get_value_range', 'meeting_rooms', 'meeting_masks',
           'post_process_rooms', 'write_post_dataset', 'get_dset', 'get_directory_name']
