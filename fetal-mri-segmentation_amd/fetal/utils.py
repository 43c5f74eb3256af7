"""From a folder of scans to a data file (reference fetal/utils.py:11-43): `fetch_training_data_files`, `create_data_file`,
`get_last_model_path`.  A scans folder holds one sub-folder per subject with `<modality>.nii<ext>`, `truth.nii<ext>` and, when the
config names weight masks, `<mask>.nii<ext>`."""
import glob
import os

import fetal_net.preprocess
from fetal_net.data import save_norm_params, write_data_to_file


def fetch_training_data_files(config, return_subject_ids=False):
    """one tuple of file names per subject folder of config["scans_dir"], the folders sorted by name: training_modalities, then "truth",
    then the names of config["weight_mask"] (None: no mask)"""
    training_data_files, subject_ids = [], []
    names = config["training_modalities"] + ["truth"] + (config["weight_mask"] if config["weight_mask"] is not None else [])
    for subject_dir in sorted(glob.glob(os.path.join(config["scans_dir"], "*")), key=os.path.basename):
        subject_ids.append(os.path.basename(subject_dir))
        training_data_files.append(tuple(os.path.join(subject_dir, name + ".nii" + config["ext"]) for name in names))
    return (training_data_files, subject_ids) if return_subject_ids else training_data_files


def create_data_file(config, device=None):
    """config["data_file"] from the scans of config["scans_dir"] (`fetal_net.data.write_data_to_file`: `normalization`, optional
    `scale_data` and `preproc`, the name of a filter of `fetal_net.preprocess`) and `norm_params.json` in config["base_dir"].
    `device` (not in the reference): where the volumes are prepared, as in `write_data_to_file`.  Returns (mean, std)."""
    training_files, subject_ids = fetch_training_data_files(config, return_subject_ids=True)
    preproc = config.get("preproc", None)
    preproc_func = getattr(fetal_net.preprocess, preproc) if preproc is not None else None
    _, (mean, std) = write_data_to_file(training_files, config["data_file"], subject_ids=subject_ids, normalize=config["normalization"],
                                        scale=config.get("scale_data", None), preproc=preproc_func, device=device)
    save_norm_params(config["base_dir"], mean, std)
    return mean, std


def get_last_model_path(model_file_path):
    """the newest of `model_file_path*.h5` by modification time"""
    return sorted(glob.glob(model_file_path + "*.h5"), key=os.path.getmtime)[-1]
