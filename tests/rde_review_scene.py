"""
The seeded scene of the RDE review-folder tests, shared by tests/golden/gen_rde_review_golden_from_reference.py (which ran the
real reference on it) and the tests (which regenerate it from the same seed, so that no image file is committed): two
cameras of 12 images of 160 x 120 -- seeded noise plus shapes, written by Pillow -- with boxes planted at the same places,
and the results file that names them.  `variety` swaps some files for the kinds the device leg must tell apart: 4:2:0 at
quality 75 and 90, one 4:2:2 file, one grayscale file, one with EXIF orientation 6, one PNG and one progressive JPEG.
"""

import os

import numpy as np

WIDTH, HEIGHT = 160, 120
CAMERAS = ('camA', 'camB')
IMAGES_PER_CAMERA = 12
#: per camera its planted spots: (x, y, w, h) normalised, category
SPOTS = {'camA': (((0.125, 0.2, 0.275, 0.35), '1'), ((0.55, 0.45, 0.3, 0.4), '2')),
         'camB': (((0.3, 0.25, 0.35, 0.3), '1'), ((0.78, 0.7, 0.3, 0.35), '1'))}      # the second leaves the image
#: the thin scene: one camera whose only spot is 200 : 1 -- a crop of 128 x 1 pixels, whose tile would be 96 x 0
THIN_BOX = (0.1, 0.4942, 0.8, 0.004)


def r3(v):
    return round(float(v), 3)


def picture(rng, k):
    """noise plus shapes: a gradient, a disc and a bar that move with k"""
    from PIL import Image, ImageDraw
    yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH]
    base = np.stack([xx * 255 // WIDTH, yy * 255 // HEIGHT, (xx + yy) * 255 // (WIDTH + HEIGHT)], axis=2).astype(np.int32)
    noisy = np.clip(base + rng.integers(-40, 41, base.shape), 0, 255).astype(np.uint8)
    image = Image.fromarray(noisy)
    draw = ImageDraw.Draw(image)
    draw.ellipse([20 + 5 * k, 30, 60 + 5 * k, 70], fill=(250, 220, 40))
    draw.rectangle([90, 10 + 4 * k, 150, 24 + 4 * k], fill=(30, 60, 200))
    return image


def file_name(camera, k, variety):
    return '{}/I{:02d}.{}'.format(camera, k, 'png' if variety and camera == 'camA' and k == 5 else 'jpg')


def write_image(image, path, camera, k, variety):
    """plain: 4:2:0 at quality 75 (camA) or 90 (camB); with variety some files are of another kind"""
    quality = 75 if camera == 'camA' else 90
    if variety and camera == 'camA':
        if k == 3:
            return image.save(path, quality=quality, subsampling=1)                       # 4:2:2
        if k == 4:
            return image.convert('L').save(path, quality=quality)                        # grayscale
        if k == 5:
            return image.save(path)                                                      # PNG
        if k == 6:
            return image.save(path, quality=quality, progressive=True)
        if k == 7:
            from PIL import Image
            exif = Image.Exif()
            exif[274] = 6
            return image.transpose(Image.ROTATE_90).save(path, quality=quality, exif=exif)     # turned back by load_image
    image.save(path, quality=quality)


def make_scene(folder, variety=False, seed=2024, thin=False):
    """Writes the images below `folder` and returns the results (the dict of a results file).  thin: the one-camera scene of
    THIN_BOX (5 images) instead."""
    rng = np.random.default_rng(seed)
    images = []
    cameras = ('thin',) if thin else CAMERAS
    for camera in cameras:
        os.makedirs(os.path.join(folder, camera), exist_ok=True)
        for k in range(5 if thin else IMAGES_PER_CAMERA):
            name = file_name(camera, k, variety)
            write_image(picture(rng, k), os.path.join(folder, name), camera, k, variety)
            dets = []
            if thin:
                dets.append({'category': '1', 'conf': r3(0.9 - 0.1 * k), 'bbox': list(THIN_BOX)})
            else:
                for s, ((x, y, w, h), category) in enumerate(SPOTS[camera]):
                    if (k + s) % 6 == 5:                          # the spot is empty in some images
                        continue
                    jx, jy = rng.integers(-2, 3, 2) / 1000.0
                    dets.append({'category': category, 'conf': r3(rng.uniform(0.3, 0.95)), 'bbox': [r3(x + jx), r3(y + jy), w, h]})
                # and one box of its own per image
                w, h = r3(rng.uniform(0.1, 0.3)), r3(rng.uniform(0.1, 0.3))
                dets.append({'category': '1', 'conf': r3(rng.uniform(0.2, 0.9)), 'bbox': [r3(rng.uniform(0, 1 - w)), r3(rng.uniform(0, 1 - h)), w, h]})
            images.append({'file': name, 'detections': dets})
    return {'info': {'format_version': '1.4', 'detector': 'seeded'},
            'detection_categories': {'1': 'animal', '2': 'person', '3': 'vehicle'}, 'images': images}


#: golden option set -> (scene is the thin one, review options that differ from the defaults)
OPTION_SETS = {
    'defaults': (False, {}),
    'primary_left': (False, {'detectionTilesPrimaryImageLocation': 'left'}),
    'primary_width_100': (False, {'detectionTilesPrimaryImageWidth': 100}),
    'grid_width_90_pixels': (False, {'detectionTilesCroppedGridWidth': 90}),
    'max_crops_3': (False, {'detectionTilesMaxCrops': 3}),
    'no_tiles': (False, {'bRenderDetectionTiles': False}),
    'thin_first_box': (True, {}),
}
OCCURRENCE_THRESHOLD = 4
#: the samples deleted before the removal pass, by position among the sorted sample names
DELETED = (0, 2)
