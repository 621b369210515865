"""A small synthetic dataset directory in the reference's on-disk format
(dataset JSON + iLED_<n>.tif 16-bit frames), shared by the loader and CLI
tests.  Frames are random uint16 with a per-frame background level, so the
background windows, the bgThresh clamp and the darkfield divide all act.
"""
from __future__ import annotations

import json
import os

import numpy as np

from fpm_amd import host

KEYS = {
    "filePrefix": "iLED_", "fileExtension": ".tif", "cropSizeX": 32, "pixelSize": 6.5,
    "objectiveMag": 8.1485, "objectiveNA": 0.1, "maxIlluminationNA": 0.2, "lambda": 0.6292,
    "cropX": 20, "cropY": 12, "bk1cropX": 1, "bk1cropY": 62, "bk2cropX": 70, "bk2cropY": 62,
    "bgThresh": 3000, "darkfieldExpMultiplier": 3, "delta1": 10, "delta2": 3,
    "arrayRotation": 0, "flipDatasetX": False, "flipDatasetY": False,
}
FRAME = (96, 104)        # height, width
N_FILES = 293            # LED numbers 1..N_FILES present on disk (all of dogStomach)


def make_dataset(root: str, seed: int = 7, keys: dict | None = None, frame_builder=None, leds=None) -> dict:
    """Write dataset.json + frames under `root`; returns the keys and frames
    ({led number: uint16 [H][W]}).  `leds`: the LED numbers to write a file for
    (default: all N_FILES); `frame_builder(led)`: that LED's frame (default: the
    random frames described above)."""
    os.makedirs(root, exist_ok=True)
    k = dict(KEYS, **(keys or {}))
    k["datasetRoot"] = root.rstrip("/") + "/"
    rng = np.random.default_rng(seed)
    frames = {}
    for led in (range(1, N_FILES + 1) if leds is None else leds):
        if frame_builder is not None:
            f = np.ascontiguousarray(frame_builder(led), np.uint16)
            frames[led] = f
            host.write_tiff16(os.path.join(root, f"iLED_{led}.tif"), f)
            continue
        bg = int(rng.integers(200, 3000))          # some frames clamp at bgThresh
        f = bg + rng.integers(0, 3000, FRAME)
        f[10:60, 15:70] += rng.integers(0, 20000, (50, 55))   # object region over the crops
        f = np.clip(f, 0, 65535).astype(np.uint16)
        frames[led] = f
        host.write_tiff16(os.path.join(root, f"iLED_{led}.tif"), f)
    text = host.dataset_json(k, host.dogstomach_led_table())
    with open(os.path.join(root, "dataset.json"), "w") as fh:
        fh.write(text)
    return dict(keys=k, frames=frames, json=os.path.join(root, "dataset.json"))


def central_leds(n_bright: int = 4, n_dark: int = 4, objective_na: float = KEYS["objectiveNA"],
                 max_na: float = KEYS["maxIlluminationNA"]):
    """LED numbers of the dogStomach table nearest the axis, n_bright of them
    brightfield and n_dark darkfield (objective NA < NA < max NA, clear of
    both limits), in LED order; and {led: darkfield}."""
    xyz = host.dogstomach_led_table().astype(np.float64)
    na = np.hypot(np.sin(np.arctan2(xyz[:, 0], xyz[:, 2])), np.sin(np.arctan2(xyz[:, 1], xyz[:, 2])))
    by_na = np.argsort(na, kind="stable")
    bright = [int(i) + 1 for i in by_na if na[i] < objective_na - 0.01][:n_bright]
    dark = [int(i) + 1 for i in by_na if objective_na + 0.01 < na[i] < max_na - 0.01][:n_dark]
    assert len(bright) == n_bright and len(dark) == n_dark
    return sorted(bright + dark), {led: led in dark for led in bright + dark}


def make_case_dataset(root: str, case, np_: int, leds=None):
    """The dataset directory of one edge case of tests/preprocess_cases.py that
    the JSON can express (integer multiplier and threshold, one patch, the
    darkfield flags from the LEDs' NA): one TIFF per LED of central_leds().
    Returns make_dataset's dict plus leds, dark ({led: flag}) and inputs (the
    case's Inputs, frame j for leds[j]); the patch is the case's first."""
    if leds is None:
        leds = central_leds()
    nums, dark = leds
    inp = case.inputs(np_, len(nums), dark=[dark[led] for led in nums])
    mult, thresh = int(inp.dark_mult), int(inp.bg_threshold)
    assert mult == inp.dark_mult and thresh == inp.bg_threshold, "not expressible in the dataset JSON"
    keys = {"cropSizeX": np_, "cropX": inp.patches[0][0], "cropY": inp.patches[0][1],
            "bk1cropX": inp.bk1[0], "bk1cropY": inp.bk1[1], "bk2cropX": inp.bk2[0], "bk2cropY": inp.bk2[1],
            "bgThresh": thresh, "darkfieldExpMultiplier": mult}
    ds = make_dataset(root, keys=keys, frame_builder=lambda led: inp.frames[nums.index(led)], leds=nums)
    return dict(ds, leds=nums, dark=dark, inputs=inp)


def dump_keys(k: dict) -> str:
    return json.dumps(k, sort_keys=True)
