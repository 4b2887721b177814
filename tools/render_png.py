"""python tools/render_png.py <scene> <w> <h> <spp> <bounces> <out.png> [--denoise] — render through the product path and write the
display image; --denoise: the AOV pass over the same samples and the default filter, the denoised display image instead."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rsoderh_raytracing_amd as R
from rsoderh_raytracing_amd import host
denoise = "--denoise" in sys.argv
args = [a for a in sys.argv[1:] if a != "--denoise"]
name, w, h, spp, mb, out = args[0], int(args[1]), int(args[2]), int(args[3]), int(args[4]), args[5]
sc = R.Scene.load_toml(os.path.join(ROOT, 'tests', 'golden', 'assets', 'scenes', name + '.toml'))
st = R.State.new(sc, R.Environment.synthetic(2048, 1024), w, h); st.max_bounces = mb
st.render_samples(spp, aov=denoise)
if denoise:
    st.denoise(download=False)
    host.write_png(out, st.denoised_display_srgb8())
else:
    host.write_png(out, st.display_srgb8())
g = st.stats(); print(name, 'kernel ms', g['kernel_ms'], 'rays', g['ext_rays'] + g['shadow_rays'])
