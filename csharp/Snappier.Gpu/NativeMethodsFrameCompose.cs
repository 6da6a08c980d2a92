// P/Invoke surface of libsnappier_hip_frame_compose.so -- one declaration per function of include/snappier_hip_frame_compose.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameCompose
{
    private const string Lib = "snappier_hip_frame_compose";                    // libsnappier_hip_frame_compose.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    // ---- batch, device pointers (asynchronous on the context's stream): new framed streams made of windows of old ones kept with their index, out of place
    // (the five dIdx* pointers are the arrays NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes, the four dSeg* the segment list -- dSegStream holds uint --,
    //  the five dNew* the index of the OUTPUTS; dOutBound may be IntPtr.Zero)
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_compose_indexed_workspace(uint nstreams, uint nout, uint nsegs, uint maxSlots, ulong stageCap, uint chunkBytes, uint maxEntries);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_compose_indexed_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, ulong nentries, IntPtr dSegFirst, IntPtr dSegStream, IntPtr dSegOff, IntPtr dSegLen, uint nout, uint nsegs, uint chunkBytes, uint maxSlots, ulong stageCap, uint maxEntries, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dNewFirst, IntPtr dNewStart, IntPtr dNewPos, IntPtr dNewTotal, IntPtr dNewTail, IntPtr dOutBound, IntPtr dWork, IntPtr dResult);
}
