"""`get_training_and_validation_generators` with the reference's arguments (reference fetal_net/generator.py:58-146) over the device
sampler of `fetal_net.device_generator`: the split is drawn or re-loaded with `fetal_net.data.get_validation_split`, the step counts
are the reference's, and the two generators are `device_data_generator`s that yield CUDA tensors.

Both generators draw from ONE `DeviceDataFile` over the union of the training and validation indices.  It is built when the first
batch of either generator is asked for: the split pickles and the step counts come out on a machine without a GPU, and the cohort is
padded and uploaded once.  The reference's host-side patch code (`data_generator`, `add_data`, `convert_data`, ...) is not restated
here; `device_generator` is this package's form of it."""
import threading

from .data import get_validation_split, split_list  # noqa: F401  (reference generator.py:158-190)
from .device_generator import DeviceDataFile, device_data_generator, list_generator, random_list_generator  # noqa: F401

__all__ = ["get_training_and_validation_generators", "get_validation_split", "split_list", "random_list_generator", "list_generator"]


class SharedDeviceDataFile(object):
    """builds the `DeviceDataFile` of several generators at its first use and hands every one of them the same object (`.ddf`)"""

    def __init__(self, data_file, patch_shape, samples_pad, truth_downsample, indices, device, distance_masks):
        self._args = (data_file, patch_shape, samples_pad, truth_downsample)
        self._kw = dict(indices=sorted(set(indices)), device=device, distance_masks=distance_masks)
        self.ddf = None
        self._lock = threading.Lock()                        # fit_generator pulls the training batches on a producer thread

    def get(self):
        with self._lock:
            if self.ddf is None:
                self.ddf = DeviceDataFile(*self._args, **self._kw)
            return self.ddf


class LazyDeviceGenerator(object):
    """iterator over the batches of `device_data_generator(shared.get(), **kwargs)`, which is made at the first `next()`;
    `.device_data_file` is the shared `DeviceDataFile` (None before any generator has asked for a batch)"""

    def __init__(self, shared, kwargs):
        self._shared, self._kwargs, self._gen = shared, kwargs, None

    @property
    def device_data_file(self):
        return self._shared.ddf

    def __iter__(self):
        return self

    def __next__(self):
        if self._gen is None:
            self._gen = device_data_generator(self._shared.get(), **self._kwargs)
        return next(self._gen)


def get_training_and_validation_generators(data_file, batch_size, n_labels, training_keys_file, validation_keys_file, test_keys_file,
                                           patch_shape=None, data_split=0.8, overwrite=False, labels=None, augment=None,
                                           validation_batch_size=None, skip_blank_train=True, skip_blank_val=False, truth_index=-1,
                                           truth_size=1, truth_downsample=None, truth_crop=True, patches_per_epoch=1, categorical=True,
                                           is3d=False, prev_truth_index=None, prev_truth_size=None, drop_easy_patches_train=False,
                                           drop_easy_patches_val=False, samples_pad=3, val_augment=None, *, device="cuda", noise_seed=0,
                                           distance_masks=None, prefetch=0):
    """-> (training generator, validation generator, training steps, validation steps), the reference's names, order and defaults.
    steps = patches_per_epoch // batch size (the validation count with `validation_batch_size`, which defaults to `batch_size`).  The
    training generator takes `augment`, `skip_blank_train` and `drop_easy_patches_train`, the validation generator `val_augment`,
    `skip_blank_val` and `drop_easy_patches_val`; everything else is shared.

    Keyword-only additions: `device`, `distance_masks` and `prefetch` as in `device_data_generator`; `noise_seed` seeds the training
    generator's in-kernel noise, `noise_seed + 1` the validation generator's.  `truth_downsample` > 1 is refused, as in
    `device_data_generator`: no model of this package produces a down-sampled output."""
    if truth_downsample is not None and truth_downsample > 1:
        raise NotImplementedError("truth_downsample is not part of the device generator")
    if patch_shape is None:
        raise ValueError("the device generator samples patches; patch_shape is required")
    if not validation_batch_size:
        validation_batch_size = batch_size
    training_list, validation_list, test_list = get_validation_split(data_file, data_split=data_split, overwrite=overwrite,
                                                                     training_file=training_keys_file,
                                                                     validation_file=validation_keys_file, test_file=test_keys_file)
    ids = getattr(data_file.root, "subject_ids", None)

    def names(items):
        return [i if ids is None else (ids[i].decode() if isinstance(ids[i], bytes) else str(ids[i])) for i in items]
    print("Training: {}".format(names(training_list)))
    print("Validation: {}".format(names(validation_list)))
    print("Test: {}".format(names(test_list)))
    num_training_steps = patches_per_epoch // batch_size
    print("Number of training steps: ", num_training_steps)
    num_validation_steps = patches_per_epoch // validation_batch_size
    print("Number of validation steps: ", num_validation_steps)

    shared = SharedDeviceDataFile(data_file, patch_shape, samples_pad, truth_downsample, list(training_list) + list(validation_list),
                                  device, distance_masks)
    common = dict(n_labels=n_labels, labels=labels, patch_shape=patch_shape, truth_index=truth_index, truth_size=truth_size,
                  truth_downsample=truth_downsample, truth_crop=truth_crop, categorical=categorical, is3d=is3d,
                  prev_truth_index=prev_truth_index, prev_truth_size=prev_truth_size, samples_pad=samples_pad, device=device,
                  prefetch=prefetch)
    training_generator = LazyDeviceGenerator(shared, dict(common, index_list=training_list, batch_size=batch_size, augment=augment,
                                                      skip_blank=skip_blank_train, drop_easy_patches=drop_easy_patches_train,
                                                      noise_seed=noise_seed))
    validation_generator = LazyDeviceGenerator(shared, dict(common, index_list=validation_list, batch_size=validation_batch_size,
                                                        augment=val_augment, skip_blank=skip_blank_val,
                                                        drop_easy_patches=drop_easy_patches_val, noise_seed=noise_seed + 1))
    return training_generator, validation_generator, num_training_steps, num_validation_steps
