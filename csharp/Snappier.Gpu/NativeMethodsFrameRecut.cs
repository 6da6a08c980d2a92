// P/Invoke surface of libsnappier_hip_frame_recut.so -- one declaration per function of include/snappier_hip_frame_recut.h, same order.
// That library is linked against libsnappier_hip.so and takes its contexts (NativeMethods.snp_ctx_create).
using System;
using System.Runtime.InteropServices;

namespace Snappier.Gpu;

internal static unsafe class NativeMethodsFrameRecut
{
    private const string Lib = "snappier_hip_frame_recut";                      // libsnappier_hip_frame_recut.so
    private const CallingConvention Cc = CallingConvention.Cdecl;

    internal const uint RewriteAll = 1;                                         // SNP_RECUT_REWRITE_ALL

    // ---- batch, device pointers (asynchronous on the context's stream): framed streams kept with their index brought to the pieces of a cut list, out of place
    // (the five dIdx* pointers are the arrays NativeMethodsFrameIndex.snp_frame_read_indexed_batch takes, dCutFirst / dCuts / ncuts the list as
    // NativeMethodsFrameCuts.snp_frame_encode_cuts_batch takes it, the five dNew* the index of the new streams; dOutBound may be IntPtr.Zero; dResult holds 8 values)
    [DllImport(Lib, CallingConvention = Cc)] internal static extern ulong snp_frame_recut_indexed_workspace(uint nstreams, uint maxSlots, ulong stageCap, uint maxEntries);
    [DllImport(Lib, CallingConvention = Cc)] internal static extern SnpStatus snp_frame_recut_indexed_batch(IntPtr ctx, IntPtr dIn, IntPtr dInOff, IntPtr dInLen, uint nstreams, IntPtr dIdxFirst, IntPtr dIdxStart, IntPtr dIdxPos, IntPtr dIdxTotal, IntPtr dIdxTail, ulong nentries, IntPtr dCutFirst, IntPtr dCuts, ulong ncuts, uint flags, uint maxSlots, ulong stageCap, uint maxEntries, IntPtr dOut, IntPtr dOutOff, IntPtr dOutCap, IntPtr dOutLen, IntPtr dStatus, IntPtr dNewFirst, IntPtr dNewStart, IntPtr dNewPos, IntPtr dNewTotal, IntPtr dNewTail, IntPtr dOutBound, IntPtr dWork, IntPtr dResult);
}
